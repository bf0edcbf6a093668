// conv_halo_rf5_kernel: the halo-tiled 5x5 convolution with the FILTERS RESIDENT IN REGISTERS -- branch5x5_2 (48 -> 64, pad 2) of the
// Inception-A blocks Mixed_5b..5d, forward and data gradient.  The 3x3 kernel of conv_halo_rf.hip carried over to taps that are no whole
// MFMA steps.
//
// Same shape as conv_halo_rf_kernel: FOUR waves, one per SIMD, wave = (filter class wc, pixel half wp), 16 x 2 filters per class (<= 64
// produced channels) over the whole reduction times 128 pixels (four rows of the 8 x 32 tile = 8 pixel fragments, 16 accumulators).  The LDS
// image is the halo of ONE tile and all its channels -- (8 + 4) x (32 + 4) = 432 pixels, filled by LDS-DMA with out-of-image rows as
// out-of-range buffer offsets, double-buffered across items -- so the only barrier is one hand-over per tile.  Fragment reads and MFMAs are
// inline asm with a rolling window of reads and hand-counted lgkmcnt, the next halo's transfers sit between the MFMAs of the tile's first
// half, the bias sits in LDS behind the halo buffers (all as there; the code the two share is conv_halo_rf.h, rf:: below).
//
// What is new: THE REDUCTION IS WALKED DENSELY.  A tap has CPT = 5..8 chunks of 8 channels (40..64 reduction channels), so a 32-channel
// MFMA step (4 chunks, one per lane group g4) does not end where a tap ends.  Padding every tap to 64 channels would cost 50 steps for the
// 48-channel layers; the dense walk over the 25 CPT chunks of (tap, chunk in tap) -- the order the packed bank already has -- takes
// ceil(25 CPT / 4) = 32 | 38 | 44 | 50 steps, two filter fragments each: 256..400 registers of filters beside 64 accumulator registers.
//   filters: a lane's fragment of step ks is chunk 4 ks + g4 of its channel's bank row; chunks past 25 CPT load as zeros.
//   pixels:  chunk q of fragment j sits at rf5_off(q, j) from the lane's base.  Within a step the four lane groups read chunks q0 .. q0 + 3:
//            in one tap these are 16 bytes apart (folded into the lane's base), and where the step straddles two taps the groups
//            g4 >= SP sit a constant K further (one pixel to the right, or the first pixel of the next halo row, less the CPT chunks
//            walked).  So a step is one immediate offset plus, for the straddling ones, a select and an add per step (3 VALU
//            instructions for 16 MFMAs) instead of a base register per (SP, K) pair: CPT = 5 and 7 have six such pairs.
//            The absent chunks of the last step (their filters are zero) read the same lane group's chunk of the step before
//            (K = -64: the same tap, a written chunk): 0 x finite.  A pad chunk is never read: 0 x NaN would be NaN.
// Pitch: 6 chunks (96 bytes) for CPT <= 6, 10 chunks (160 bytes) for CPT 7 and 8.  ds_read_b128 serves the lanes in groups of 16 made of
// pixels {0-3, 12-15} of one lane group and pixels {4-11} of the next (MI355X LDS): with a pitch of P chunks their 16-byte slots are
// (pixel P + chunk) mod 16, and P = 6 and P = 10 (P / 2 odd) give each half of such a group eight distinct slots of one parity, the
// neighbouring chunk the other parity: conflict-free in every whole-tap step and wherever SP = 2 (CPT = 6: the pairs of lane groups that
// share a read cycle, (0, 1) and (2, 3), each stay in one tap).  With CPT = 5 and 7 a straddle inside a pair (SP = 1 | 3) shifts the second
// group by K / 16 = (even) - CPT slots, an odd number: those steps, two or three in every five | seven, are two-way.  An odd pitch
// (5, 7, 9) is two-way in every step.  Two buffers: 82 KB | 136 KB.
// The halo plan keeps 16 bits per transfer (halo row, column, chunk) and forms the byte offset when the transfer is issued: at 400
// filter registers a stored offset per transfer (17) does not fit, and with 16 MFMAs per step the extra VALU instructions are free.
//
// Data gradient (64 -> 48 in the backbone): the same walk over the transposed bank with the taps backwards from the far corner of the
// halo; 64 reduction channels are two whole steps per tap, nothing straddles.  The 48 produced channels sit on the same two classes of 32
// (the second class half empty: a quarter of the MFMAs multiply zeros; three row tiles per wave would be 600 filter registers, and an
// uneven or tap-split layout an exchange through LDS that has no room, below).  The ReLU mask travels by LDS-DMA into wave-private
// regions behind the halo buffers, issued after the halo's transfers, and holds only the chunks of a class's REAL channels (4 per pixel
// in the first class, (cprod - 32) / 8 in the second): with the 160-byte pitch the two halo buffers take 136 KB, so the LDS has room
// for the mask of <= 48 produced channels -- 64 -> 48 fills its 160 KB to the byte -- and a masked launch with 56 | 64 reduction AND
// more than 48 produced channels is not eligible.  ACCUM loads one pixel fragment at a time and stays off in the planner.
#include "din_common.h"
#include "conv_wgrad.h"
#include "conv_gather.h"
#include "conv_shared.h"
#include "conv_halo_rf.h"

using din_wgrad::lds_dma16;
using din_gather::ConvK;
namespace rf = din_rf;

namespace {

constexpr int R5_HWW = rf::TW + 4, R5_HWH = rf::TH + 4, R5_HPX = R5_HWW * R5_HWH;
constexpr int R5_TI = 2;                                                          // 16-row filter tiles per wave: two classes, <= 64 produced channels
constexpr int r5_pch(int cpt) { return cpt <= 6 ? 6 : 10; }                       // pitch in chunks (header: bank conflicts)
constexpr int r5_nwt(int cpt) { return (R5_HPX * r5_pch(cpt) + 63) / 64; }        // 1 KB wave-transfers of one halo
constexpr int r5_hb(int cpt) { return r5_nwt(cpt) * 1024; }                       // bytes of one halo buffer
// dynamic LDS: two halo buffers, then the four waves' bias values (forward) or their mask regions (masked data gradient): a wave's region
// holds its 128 pixels x the chunks of its class's real channels -- 4 in the first class, (cprod - 32) / 8 in the second
constexpr int r5_n1(int cprod) { return (cprod - 32 + 7) / 8; }
constexpr size_t r5_lds(int cpt, bool dg, bool mask, int cprod) {
    return (size_t)2 * r5_hb(cpt) + (dg ? (mask ? (size_t)2 * 2048 * (4 + r5_n1(cprod)) : 0) : 1024);
}
constexpr size_t R5_LDS_MAX = 160 * 1024;

// ---- the dense walk.  Chunk q = tap * CPT + c of the reduction; step ks covers chunks 4 ks .. 4 ks + 3, one per lane group.
// byte offset of chunk q of pixel fragment j (row j >> 1 of the wave's four, columns (j & 1) * 16 ..) from the lane's base
// (the data gradient walks the taps backwards from the far corner of the halo)
template <int CPT, bool DG>
constexpr int r5_off(int q, int j) {
    const int tap = q / CPT, c = q - tap * CPT, r = tap / 5, s = tap - r * 5;
    const int ry = DG ? 4 - r : r, sx = DG ? 4 - s : s;
    return (((j >> 1) + ry) * R5_HWW + (j & 1) * 16 + sx) * (r5_pch(CPT) * 16) + c * 16;
}
// the chunk lane group g reads in step ks: absent ones (past the reduction) read the group's chunk of the step before
template <int CPT>
constexpr int r5_chunk(int ks, int g) { return 4 * ks + g < 25 * CPT ? 4 * ks + g : 4 * ks + g - 4; }
// what group g's chunk lies beyond a whole-tap step's (16 bytes per group from the first one's)
template <int CPT, bool DG>
constexpr int r5_delta(int ks, int g) { return r5_off<CPT, DG>(r5_chunk<CPT>(ks, g), 0) - r5_off<CPT, DG>(4 * ks, 0) - 16 * g; }
// first lane group of step ks that sits K further (4: none), and K
template <int CPT, bool DG>
constexpr int r5_sp(int ks) {
    for (int g = 1; g < 4; ++g) if (r5_delta<CPT, DG>(ks, g) != 0) return g;
    return 4;
}
template <int CPT, bool DG>
constexpr int r5_k(int ks) { return r5_sp<CPT, DG>(ks) < 4 ? r5_delta<CPT, DG>(ks, r5_sp<CPT, DG>(ks)) : 0; }
// every step is of that form, and no read leaves the tap's real chunks
template <int CPT, bool DG>
constexpr bool r5_walk_ok() {
    for (int ks = 0; ks < (25 * CPT + 3) / 4; ++ks)
        for (int g = 0; g < 4; ++g) {
            if (r5_delta<CPT, DG>(ks, g) != (g >= r5_sp<CPT, DG>(ks) ? r5_k<CPT, DG>(ks) : 0)) return false;
            if (r5_chunk<CPT>(ks, g) < 0 || r5_chunk<CPT>(ks, g) >= 25 * CPT) return false;
        }
    return true;
}

// CPT: 16-byte chunks (8 channels) per tap of the reduction; DG: data gradient (taps walked backwards)
template <int CPT, bool DG>
__global__ __launch_bounds__(256, 1) void conv_halo_rf5_kernel(ConvK p) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(CPT >= 5 && CPT <= 8 && r5_walk_ok<CPT, DG>(), "dense walk");
    constexpr int TI = R5_TI;
    constexpr int PCH = r5_pch(CPT), PB = PCH * 16, NWT = r5_nwt(CPT), HB = r5_hb(CPT);
    constexpr int NTR = (NWT + 3) / 4;                                            // halo transfers per wave (the last one not for every wave)
    constexpr int Q = 25 * CPT, NSTEP = (Q + 3) / 4, NF = NSTEP * 8;              // chunks, steps, pixel fragments read per tile
    constexpr int NA = (256 - 32 * TI) / 4;                                       // filter fragments in accumulation registers (beside the 32 TI accumulator registers)
    constexpr int D = 4;                                                          // fragment reads in flight ahead of the MFMAs
    constexpr int SP = 8;                                                         // fragments between two transfers: one per step, all in the tile's first half
    constexpr int NTR_M = 4 * TI;                                                 // mask transfers per wave, at most (128 pixels x <= 2 TI chunks)
    static_assert(NTR * SP <= NF / 2 + 8 && (NTR + NTR_M) * SP <= NF, "every transfer has a slot, the halo's in the tile's first half");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, g4 = lane >> 4;
    const int wc = wid & 1, wp = wid >> 1;
    const int cbase = wc * 16 * TI;                                               // first produced channel of the wave's class
    const uint32_t lds_base = (uint32_t)(uintptr_t)smem_raw;
    const uint32_t ldsWv = __builtin_amdgcn_readfirstlane(lds_base + (uint32_t)(wid * 1024));
    // the wave's mask region: mch chunks per pixel (its class's real channels), the first class's regions first
    const int mch = __builtin_amdgcn_readfirstlane(wc == 0 ? 2 * TI : (p.Cout - 16 * TI + 7) >> 3);
    const uint32_t ldsMk = __builtin_amdgcn_readfirstlane(lds_base + (uint32_t)(2 * HB + (wc == 0 ? wp * 2048 * 2 * TI : 2 * 2048 * 2 * TI + wp * 2048 * mch)));

    // the launch's geometry in registers: nothing below reads the argument block again (a scalar load inside the walk would share lgkmcnt
    // with the counted fragment reads)
    const int W_ = p.W, H_ = p.H, ldi = p.ldi, OH = p.OH, OW = p.OW, Cout = p.Cout, ldo = p.ldo, cooff = p.cooff, flags = p.flags;
    const int ldm = p.ldm, moff = p.moff, cioff2 = p.cioff * 2;
    const int hy0 = p.by - (DG ? 4 : 0), hx0 = p.bx - (DG ? 4 : 0);
    const int tiles_x = (OW + rf::TW - 1) / rf::TW, tiles_y = (OH + rf::TH - 1) / rf::TH;
    const int tiles_img = tiles_x * tiles_y, nitems = tiles_img * p.NB;
    const long long img_bytes = (long long)H_ * W_ * ldi * 2ll;
    const long long oimg_bytes = (long long)OH * OW * ldo * 2ll, mimg_bytes = (long long)OH * OW * ldm * 2ll;
    const char* const inp = reinterpret_cast<const char*>(p.in);
    char* const outp = reinterpret_cast<char*>(p.out);
    const char* const maskp = reinterpret_cast<const char*>(p.mask);
    const bool masked = DG && (flags & DIN_CONV_MASK) != 0;

    using rf::Item;
    // ---- halo transfers.  Halo chunk id = (wid + 4 i) * 64 + lane of transfer i, lane-linear in LDS.  What a lane fetches in transfer i
    // never changes: pk keeps its halo column (6 bits), chunk (4 bits; 15: a pad chunk or past the halo, never fetched) and halo row (4
    // bits), 16 bits per transfer.  Rows outside the image need no test: the buffer resource covers ONE image and the whole offset sits in
    // the VGPR, so a row above it is a negative (= huge unsigned) offset and a row below it one past the image's bytes -- both out of
    // range, and such transfers land as zeros.
    uint32_t pk[(NTR + 1) / 2];
#pragma unroll
    for (int i = 0; i < (NTR + 1) / 2; ++i) pk[i] = 0u;
#pragma unroll
    for (int i = 0; i < NTR; ++i) {
        const int id = (wid + 4 * i) * 64 + lane;
        const int hp = id / PCH, cc = id - hp * PCH;
        const int hy = hp / R5_HWW, hx = hp - hy * R5_HWW;
        const bool real = hp < R5_HPX && cc < CPT;
        pk[i >> 1] |= (uint32_t)((real ? hx : 0) | ((real ? cc : 15) << 6) | ((real ? hy : 0) << 10)) << (16 * (i & 1));
    }
    // what the transfers of one item share: the image's resource, the byte offset of the halo's first pixel, the columns left of the halo
    struct HaloBlk { __amdgpu_buffer_rsrc_t rs; int base, gx0; };
    auto halo_blk = [&](const Item& it) __attribute__((always_inline)) {
        HaloBlk h;
        h.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(inp) + (long long)it.n * img_bytes, 0, (int)img_bytes, 0x00020000);
        h.gx0 = it.tx * rf::TW + hx0;
        h.base = ((it.ty * rf::TH + hy0) * W_ + h.gx0) * ldi * 2 + cioff2;
        return h;
    };
    auto halo_one = [&](int buf, const HaloBlk& h, int i) __attribute__((always_inline)) {
        if (wid + 4 * i >= NWT) return;                                           // (wave-uniform: past the buffer)
        asm volatile("" : "+v"(pk[i >> 1]));                                      // the transfer's instructions stay HERE, between the MFMAs around them
        const int hx = (int)__builtin_amdgcn_ubfe(pk[i >> 1], 16 * (i & 1), 6), cc = (int)__builtin_amdgcn_ubfe(pk[i >> 1], 16 * (i & 1) + 6, 4);
        const int hy = (int)__builtin_amdgcn_ubfe(pk[i >> 1], 16 * (i & 1) + 10, 4);
        const bool ok = (unsigned)(h.gx0 + hx) < (unsigned)W_ && cc < CPT;
        int voff = ((hy * W_ + hx) * ldi + cc * 8) * 2 + h.base;
        voff = ok ? voff : (int)rf::OOB;
        // (readfirstlane: under scalar-register pressure the allocator keeps such a uniform sum in a vector register, which m0 cannot take)
        lds_dma16(__builtin_amdgcn_readfirstlane(ldsWv + (uint32_t)(buf * HB + i * 4096)), h.rs, voff, 0);
    };
    // transfer i of the wave's own mask region: chunk id = i * 64 + lane = (pixel pl of the wave's 128, chunk c of its mch)
    auto mask_one = [&](const Item& it, int i) __attribute__((always_inline)) {
        if (i * 64 >= 128 * mch) return;                                          // (wave-uniform: past the region)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(maskp) + (long long)it.n * mimg_bytes, 0, (int)mimg_bytes, 0x00020000);
        const unsigned id = (unsigned)(i * 64 + ln), pl = id / (unsigned)mch, c = id - pl * (unsigned)mch;
        const int gy = it.ty * rf::TH + 4 * wp + (int)(pl >> 5), gx = it.tx * rf::TW + (int)(pl & 31u);
        const int co = cbase + (int)c * 8;
        const bool ok = gy < OH && gx < OW && co < Cout;
        lds_dma16(__builtin_amdgcn_readfirstlane(ldsMk + (uint32_t)(i * 1024)), rs, ok ? ((gy * OW + gx) * ldm + moff + co) * 2 : (int)rf::OOB, 0);
    };

    const int G = (int)gridDim.x;
    int item = xcd_remap((int)blockIdx.x, G);
    if (item >= nitems) return;
    Item cur = rf::decode_item(item, tiles_img, tiles_x);
    {
        const HaloBlk h0 = halo_blk(cur);
#pragma unroll
        for (int i = 0; i < NTR; ++i) halo_one(0, h0, i);
    }

    // ---- the wave's filters as A fragments, once: MFMA row m of row tile i is channel cbase + (m >> 2) * 4 TI + 4 i + (m & 3); the
    // fragment of step ks holds chunk 4 ks + g4 of that channel's bank row (zeros past the reduction)
    u32x4 Wf[NSTEP][TI];
    {
        __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, (int)p.w_bytes, 0x00020000);
        const int wld16 = p.wld * 16;
#pragma unroll
        for (int ks = 0; ks < NSTEP; ++ks)
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                const int chan = cbase + (frow >> 2) * 4 * TI + i * 4 + (frow & 3);
                const bool real = chan < Cout && ks * 4 + g4 < Q;
                Wf[ks][i] = __builtin_amdgcn_raw_buffer_load_b128(rsW, real ? chan * wld16 + g4 * 16 : (int)rf::OOB, ks * 64, 0);
            }
        // where they live is decided HERE (rf::mfma): the first NA fragments in accumulation registers, the others in architectural ones
        rf::static_for<0, NSTEP * TI>([&](auto N_) __attribute__((always_inline)) {
            constexpr int n = decltype(N_)::value;
            rf::pin<(n < NA)>(Wf[n / TI][n % TI]);
        });
    }
    // forward: the wave's 16 TI bias values behind the halo buffers
    if constexpr (!DG) {
        if (lane < 16 * TI) {
            const int co = cbase + lane;
            *reinterpret_cast<float*>(smem_raw + 2 * HB + wid * 256 + lane * 4) = ((flags & DIN_CONV_BIAS) && co < Cout) ? p.bias[co] : 0.f;
        }
    }
    f32x4 acc[TI][8];                                                             // (the first step of a tile writes them: rf::mfma<.., FIRST>)

    // lane base of the fragment reads: first row of the wave's pixel half, pixel column frow, chunk g4
    const uint32_t xb0 = lds_base + (uint32_t)((4 * wp * R5_HWW + frow) * PB + g4 * 16);
    u32x4 xf[D];

    // ---- epilogue straight from the accumulators: a lane holds channels cbase + 4 TI g4 .. + 4 TI of pixel frow of every fragment
    auto epilogue = [&](const Item& it) __attribute__((always_inline)) {
        int ln = lane;                                                             // (the lane's offsets are recomputed per item: hoisted out of the item
        asm volatile("" : "+v"(ln));                                              //  loop they cost registers the filters fill)
        const int frow_e = ln & 15, g4_e = ln >> 4;
        __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(outp + (long long)it.n * oimg_bytes, 0, (int)oimg_bytes, 0x00020000);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int gy = it.ty * rf::TH + 4 * wp + (j >> 1), gx = it.tx * rf::TW + (j & 1) * 16 + frow_e;
            const int pxo = (gy < OH && gx < OW) ? ((gy * OW + gx) * ldo + cooff) * 2 : (int)rf::OOB;   // byte offset of the fragment's pixel, or out of range
            [[maybe_unused]] u32x2 old[TI];                                       // (BIAS / RELU are forward flags, MASK / ACCUM data-gradient flags: host)
            if constexpr (DG) {
#pragma unroll
                for (int i = 0; i < TI; ++i) {
                    const int co = cbase + g4_e * 4 * TI + i * 4;
                    if (flags & DIN_CONV_ACCUM) old[i] = __builtin_amdgcn_raw_buffer_load_b64(rsO, rf::piece_off(pxo, co, Cout), 0, 0);
                }
            }
            const int pl = (j >> 1) * 32 + (j & 1) * 16 + frow_e;
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                const int co = cbase + g4_e * 4 * TI + i * 4;
                f32x4 v = acc[i][j];
                if constexpr (!DG) {
                    v += *reinterpret_cast<const f32x4*>(smem_raw + 2 * HB + wid * 256 + (g4_e * 4 * TI + i * 4) * 4);
                    if (flags & DIN_CONV_RELU) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                    }
                } else {
                    if (masked) {
                        // (a lane group past the class's real channels stores nothing: it reads the region's last chunk, not past it)
                        const int gm = g4_e < mch ? g4_e : mch - 1;
                        const u32x2 mk = *reinterpret_cast<const u32x2*>(smem_raw + (ldsMk - lds_base) + (pl * mch + gm) * 16 + i * 8);
                        rf::mask4(v, mk);
                    }
                    if (flags & DIN_CONV_ACCUM) v = rf::accum4(v, old[i]);
                }
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])}, rsO, rf::piece_off(pxo, co, Cout), 0, 0);
            }
            asm volatile("" ::: "memory");                                       // one fragment at a time: the filters leave no registers for more
        }
    };

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    int hb = 0;
    for (;;) {
        const int item_n = item + G;
        const bool hn = item_n < nitems;                                          // a next item exists: its halo goes into buffer hb ^ 1
        const Item nxt = hn ? rf::decode_item(item_n, tiles_img, tiles_x) : cur;
        const HaloBlk hnx = halo_blk(nxt);
        const uint32_t xa = xb0 + (uint32_t)(hb * HB);
        // the read address of a step: xa, or for a step that straddles two taps xa + K in the lane groups >= SP of the step (made where
        // the step's first read is issued: kept per step they would be registers the filters fill)
        uint32_t xs[2] = {xa, xa};
        auto step_addr = [&](auto S_) __attribute__((always_inline)) {
            constexpr int s = decltype(S_)::value;
            if constexpr (r5_sp<CPT, DG>(s) < 4) {
                int ln = lane;
                asm volatile("" : "+v"(ln));
                xs[s & 1] = xa + (uint32_t)(ln >= 16 * r5_sp<CPT, DG>(s) ? r5_k<CPT, DG>(s) : 0);
            } else {
                xs[s & 1] = xa;
            }
        };
        rf::static_for<0, D>([&](auto F_) __attribute__((always_inline)) {
            constexpr int f = decltype(F_)::value;
            static_assert(D <= 8 && r5_sp<CPT, DG>(0) == 4, "the first reads belong to step 0, a whole-tap step");
            rf::read<r5_off<CPT, DG>(0, f & 7)>(xf[f], xa);
        });
        rf::static_for<0, NF>([&](auto F_) __attribute__((always_inline)) {
            constexpr int f = decltype(F_)::value;
            constexpr int ks = f >> 3, j = f & 7;
            rf::wait<(NF - 1 - f < D - 1 ? NF - 1 - f : D - 1)>(xf[f % D]);
            rf::static_for<0, TI>([&](auto I_) __attribute__((always_inline)) {
                constexpr int i = decltype(I_)::value;
                rf::mfma<(ks * TI + i < NA), (ks == 0)>(acc[i][j], Wf[ks][i], xf[f % D]);
            });
            if constexpr (f + D < NF) {
                constexpr int nf = f + D, ns = nf >> 3;
                if constexpr ((nf & 7) == 0) step_addr(std::integral_constant<int, ns>{});
                rf::read<r5_off<CPT, DG>(4 * ns, nf & 7)>(xf[f % D], xs[ns & 1]);
            }
            if constexpr (f % SP == 0) {                                          // one transfer after the MFMAs of every SP-th fragment
                constexpr int t = f / SP;
                if constexpr (t < NTR) { if (hn) halo_one(hb ^ 1, hnx, t); }
                else if constexpr (DG && t - NTR < NTR_M) { if (masked) mask_one(cur, t - NTR); }
            }
        });
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");                        // (the last MFMAs' results: read by the epilogue's VALU, no hazard the compiler sees)
        // hand-over: this wave's transfers (next halo, the item's mask) have landed; the stores in flight are a tile old
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        epilogue(cur);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        hb ^= 1;
        if (!hn) break;
        item = item_n; cur = nxt;
    }
#endif
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// the instantiations, X(CPT, DG): both directions, 40 | 48 | 56 | 64 reduction channels, <= 64 produced channels
#define DIN_CONV_HALO_RF5_TABLE(X) X(5, false) X(6, false) X(7, false) X(8, false) X(5, true) X(6, true) X(7, true) X(8, true)

struct Rf5Inst { int cpt; bool dg; };

// the kernel of an instantiation as rocprofv3 prints it
std::string rf5_kernel_name(const Rf5Inst& r) {
    char s[64];
    snprintf(s, sizeof s, "conv_halo_rf5_kernel<%d, %s>", r.cpt, r.dg ? "true" : "false");
    return s;
}

// the table row of an instantiation: launched on `st` when `k` is given, only looked up otherwise; a tuple without a row is an error
int rf5_row(const Rf5Inst& r, const ConvK* k, hipStream_t st) {
    auto go = [&](auto kern) {
        if (!k) return DIN_OK;
        const int tiles = ((k->OH + rf::TH - 1) / rf::TH) * ((k->OW + rf::TW - 1) / rf::TW) * k->NB;
        const size_t lds = r5_lds(r.cpt, r.dg, (k->flags & DIN_CONV_MASK) != 0, k->Cout);
        DIN_REQUIRE(lds <= R5_LDS_MAX, "conv_halo_rf5: %zu bytes of LDS", lds);
        raise_lds_limit(kern, lds);
        hipLaunchKernelGGL(kern, dim3(tiles < 256 ? tiles : 256), dim3(256), lds, st, *k);
        return DIN_OK;
    };
#define DIN_ROW(CPT_, DG_) \
    if (r.cpt == CPT_ && r.dg == DG_) return go(conv_halo_rf5_kernel<CPT_, DG_>);
    DIN_CONV_HALO_RF5_TABLE(DIN_ROW)
#undef DIN_ROW
    DIN_FAIL(DIN_E_ARG, "conv_halo_rf5: %s is not instantiated", rf5_kernel_name(r).c_str());
}

// the planner's rule (option unset)
bool rf5_wanted(int which, int flags, int oh, int ow, int64_t M) {
    if (!rf::tile_waste_ok(oh, ow)) return false;
    // accumulate operands are requested one pixel fragment at a time (the filters leave no registers for more): exposed memory round
    // trips per tile, not measured against the old kernels -- no backbone layer asks for it
    if (flags & DIN_CONV_ACCUM) return false;
    // measured, conv_gather_fast_kernel against this one at 96 / 24 / 12 frames of 87 x 157 pixels (profiles/halo_rf5_layers.txt).  Forward
    // 48 -> 64: -46 / -35 / -26 %, each several times the rounds' spread: routed from the 12-frame launch up.  Masked data gradient
    // 64 -> 48 (a quarter of its MFMAs idle): -25 % at 96 frames; -11 % and -8 % at 24 and 12, the former inside the spread of its
    // rounds: routed at the 96-frame size only.  Below what was measured: old kernels.
    return M >= (which == 0 ? 160 * 1024 : 1280 * 1024);
}

// Eligibility, geometry and instantiation of the launch `which` (0 forward, 1 data gradient) of a descriptor: what rf::plan_common asks of
// a 5x5 with 40 .. 64 channels, and the launch's LDS within 160 KB -- a MASKED data gradient with 56 or 64 reduction channels (160-byte
// pitch: 136 KB of halo buffers) has room for the mask of <= 48 produced channels only.  Options: DIN_CONV_HALO=0 and DIN_CONV_HALO_RF5=0
// switch the kernel off, DIN_CONV_HALO_RF5=2 forces it on every eligible shape; unset, the planner's rule holds (rf5_wanted).  Reads no
// pointer.
bool rf5_plan(const din_conv_desc* d, int which, int flags, int ldm, int moff, ConvK& k, Rf5Inst& r) {
    if (!rf::plan_common(d, which, flags, ldm, moff, 5, 64, k)) return false;
    if (r5_lds(k.cpt, which == 1, (flags & DIN_CONV_MASK) != 0, k.Cout) > R5_LDS_MAX) return false;
    const char* rv = DIN_OPT("DIN_CONV_HALO_RF5");
    const int mode = rv ? atoi(rv) : 1;
    if (mode == 0 || (mode != 2 && !rf5_wanted(which, flags, k.OH, k.OW, k.M))) return false;
    r.cpt = k.cpt; r.dg = which == 1;
    return true;
}

struct Rf5 {
    typedef Rf5Inst Inst;
    static constexpr auto plan = rf5_plan;
    static constexpr auto row = rf5_row;
    static constexpr auto name = rf5_kernel_name;
    static constexpr const char* prefix = "conv_rf5";
};

}  // namespace

extern "C" {

int din_conv_rf5_eligible(const din_conv_desc* d, int which, int flags, int ldm, int moff) { return rf::eligible<Rf5>(d, which, flags, ldm, moff); }

// (workspace: the argument list of din_conv_fwd / din_conv_dgrad; this kernel never splits its reduction)
int din_conv_rf5_fwd(const din_conv_desc* d, const void* in, const void* wpk, const float* bias, void* out, int flags,
                     void* /*workspace*/, int64_t /*workspace_bytes*/, void* stream) {
    return rf::fwd<Rf5>(d, in, wpk, bias, out, flags, stream);
}

int din_conv_rf5_dgrad(const din_conv_desc* d, const void* dout, const void* wpk_t, void* din_, const void* mask, int ldm, int moff, int flags,
                       void* /*workspace*/, int64_t /*workspace_bytes*/, void* stream) {
    return rf::dgrad<Rf5>(d, dout, wpk_t, din_, mask, ldm, moff, flags, stream);
}

int din_conv_rf5_kernel_names(const din_conv_desc* d, int which, int flags, int ldm, int moff, char* buf, int buf_bytes) {
    return rf::kernel_names<Rf5>(d, which, flags, ldm, moff, buf, buf_bytes);
}

}  // extern "C"
