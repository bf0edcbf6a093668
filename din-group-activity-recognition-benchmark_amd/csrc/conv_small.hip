// Small-channel 3x3 convolution for the stem layers (Inception Conv2d_1a / 2a / 2b, forward and stride-1 data gradient; bf16): the kernel,
// the rule that decides its variant (conv_small_variant), the table of its instantiations, and the launcher and the namer that both walk
// that table.  conv_igemm.hip's choose_gather decides whether a launch runs here; the interface is in conv_gather.h.
#include "din_common.h"
#include "conv_wgrad.h"
#include "conv_gather.h"
#include "conv_shared.h"
#include <stdlib.h>

using din_wgrad::lds_dma16;
using din_gather::ConvK;
using din_gather::SmallVariant;

namespace {

template <int V> struct IcTag { static constexpr int value = V; };

// ------------------------------------------------------------------------------------------------
// Small-channel 3x3 (stem) convolution: filters stationary in LDS + input HALO tiles, persistent workgroups.
// For layers with 32/64 reduction channels and <= 64 produced channels over millions of pixels (Inception Conv2d_2a/2b, fwd and
// dgrad) the implicit-GEMM kernel is bound by the L2->CU operand stream: im2col pulls every input pixel kh*kw times.  Here
//   * the whole filter bank of the launch (<= 36 KiB) is loaded into LDS once per workgroup and stays there;
//   * per 8x32 output tile the (8+kh-1) x (32+kw-1) input halo is brought in ONCE by LDS-DMA (1.33x the unique bytes instead of 9x),
//     out-of-image pixels as hardware zeros; all taps are formed from LDS with a swizzle that is conflict-free at every pixel
//     offset ((hp>>1)&3 for 64-byte pixels, hp&7 for 128-byte pixels; brute-forced against the ds_read_b128 lane groups);
//   * workgroups are persistent (grid = 2 per CU) and walk the tiles; with 64-byte pixels the next halo is in flight while the
//     current tile is multiplied; the epilogue is staged through the just-consumed halo buffer -> 16-byte coalesced stores with the
//     usual fused bias / ReLU / ReLU-backward mask / accumulate.
// bf16 only; stride 1, dilation 1; the gather geometry (ay = 1, by, cy = +-1) covers forward and (stride-1) dgrad.
// ------------------------------------------------------------------------------------------------
// NW: waves per workgroup (4, or 8 for the two variants whose 80 KiB of LDS allow ONE workgroup per CU -- the 64-filter forward and the
// 64-channel dgrad of Conv2d_2b: eight waves give every SIMD two waves; each wave then owns two instead of four 16-pixel segments)
// EPI (dgrad launches: the host picks it when DIN_CONV_MASK / DIN_CONV_ACCUM is set): the epilogue's extra operands are requested at the top
// of the tile and held in registers through the MFMA phase; without it they are fetched inside the store loop (and cost no registers --
// compiled into the forward variants the prefetch registers slowed Conv2d_2b's forward by a third).
template <int CPP, int BN, int NBUF, int KH, int KW, int ST, bool U8 = false, int NW = 4, bool EPI = false>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 1 : 2) void conv_small_kernel(ConvK p) {
    constexpr int NTHREADS = 64 * NW;                                  // (shadows the file-level 256)
    static_assert(!U8 || NW == 4, "the uint8 halo loader is written for four waves");
    static_assert(!U8 || (CPP == 1 && NBUF == 2), "uint8 frames feed the image layer only");
#if defined(__HIP_DEVICE_COMPILE__)
    typedef bf16_t T;
    constexpr int TH = 8, TW = 32, NPX = TH * TW;
    constexpr int TI = BN / 16, TJ = 16 / NW, NTAPS = KH * KW;
    // MFMA k-slices (32 channels-of-taps each): CPP >= 4: SL slices per tap; CPP == 1 (image layer, 8 padded channels per pixel):
    // four taps share one slice, lane group g4 carries tap 4*slice + g4 (taps >= NTAPS hit zero filter chunks of the packed bank)
    constexpr int SL = CPP >= 4 ? CPP / 4 : 1, NSL = CPP >= 4 ? NTAPS * SL : (NTAPS + 3) / 4;
    constexpr int CPITCH = BN * 2 + 16;
    constexpr int HWW = (TW - 1) * ST + KW, HWH = (TH - 1) * ST + KH, HPX = HWW * HWH, HC = HPX * CPP;  // halo geometry (pixels, chunks)
    constexpr int WBYTES = NSL * BN * 4 * 16;
    constexpr int HBYTES = (HC * 16 + 1023) / 1024 * 1024;                                // whole 1-KiB DMA slots
    constexpr int NSLOT = HBYTES / 1024, NTR = (NSLOT + NW - 1) / NW;
    constexpr int NPASS = HBYTES / CPITCH >= NPX ? 1 : 2;                                  // epilogue passes through the staging buffer
    static_assert(HBYTES / CPITCH >= NPX / NPASS, "staging does not fit the halo buffer");
    constexpr int JN = TJ / NPASS;                                                         // pixel segments per wave per pass
    constexpr int CPR = BN / 8;                                                            // 16-byte chunks per produced pixel
    constexpr int NST = (NPX / NPASS) * CPR / NTHREADS * NPASS;                            // store instructions per wave per tile
    static_assert((NPX / NPASS) * CPR % NTHREADS == 0, "store loop must be uniform");
    constexpr unsigned OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    u32x4* Wl = reinterpret_cast<u32x4*>(smem_raw);
    auto swz = [](int row) { return CPP == 1 ? 0 : CPP == 4 ? ((row >> 1) & 3) : (row & 7); };

    // ---- filters: [tap][co][chunk ^ swz(co)]  (CPP == 1: [slice][co][tap & 3]) ---------------------------------------------
    {
        const u32x4* __restrict__ wp = reinterpret_cast<const u32x4*>(p.w);
        if (CPP >= 4) {
            for (int id = tid; id < NTAPS * BN * CPP; id += NTHREADS) {
                const int row = id / CPP, slot = id - row * CPP;
                const int tap = row / BN, co = row - tap * BN;
                const int cc = slot ^ swz(co);
                Wl[id] = wp[(int64_t)co * p.wld + tap * CPP + cc];
            }
        } else {
            for (int id = tid; id < NSL * BN * 4; id += NTHREADS) {
                const int row = id >> 2, g = id & 3;
                const int sl = row / BN, co = row - sl * BN;
                Wl[id] = wp[(int64_t)co * p.wld + sl * 4 + g];          // sl*4+g < wld: the packed row is zero beyond the last tap
            }
        }
    }
    // ---- halo DMA plan: transfer i of this wave covers chunk ids [(wid + 4 i) * 64, +64) ------------------------------------
    int rel[NTR];                                      // byte offset relative to the halo origin pixel (chunk already permuted)
    short hyv[NTR], hxv[NTR];
#pragma unroll
    for (int i = 0; i < NTR; ++i) {
        const int id = (wid + NW * i) * 64 + lane;
        const int hp = id / CPP, slot = id - hp * CPP;
        const int cc = slot ^ swz(hp);
        const int hy = hp / HWW, hx = hp - hy * HWW;
        rel[i] = id < HC ? (hy * p.W + hx) * p.ldi * 2 + cc * 16 : -1;
        hyv[i] = (short)hy; hxv[i] = (short)hx;
    }
    const int hy0 = p.by + (p.cy < 0 ? (KH - 1) * p.cy : 0), hx0 = p.bx + (p.cx < 0 ? (KW - 1) * p.cx : 0);   // halo origin - tile origin
    const int tiles_x = (p.OW + TW - 1) / TW, tiles_y = (p.OH + TH - 1) / TH;
    const int tiles_img = tiles_x * tiles_y, ntiles = tiles_img * p.NB;
    const long long img_bytes = (long long)p.H * p.W * p.ldi * 2ll;
    const long long oimg_bytes = (long long)p.OH * p.OW * p.ldo * 2ll, mimg_bytes = (long long)p.OH * p.OW * p.ldm * 2ll;
    const uint32_t lds_base = (uint32_t)(uintptr_t)smem_raw;
    const uint32_t ldsH0 = __builtin_amdgcn_readfirstlane(lds_base + (uint32_t)WBYTES + (uint32_t)(wid * 1024));

    auto issue_halo = [&](int buf, int tile) {
        const int n = tile / tiles_img;
        const int tr = tile - n * tiles_img;
        const int ty = tr / tiles_x, tx = tr - ty * tiles_x;
        const int gy0 = ty * TH * ST + hy0, gx0 = tx * TW * ST + hx0;
        // one image per resource: 32-bit offsets always suffice; out-of-image pixels get the out-of-range offset -> zeros
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(reinterpret_cast<const char*>(p.in)) + (long long)n * img_bytes, 0, (int)img_bytes, 0x00020000);
        const int base = (gy0 * p.W + gx0) * p.ldi * 2 + p.cioff * 2;
        const uint32_t dst = ldsH0 + (uint32_t)(buf * HBYTES);
#pragma unroll
        for (int i = 0; i < NTR; ++i) {
            if (wid + NW * i < NSLOT) {                                                  // uniform: slot inside the halo buffer
                const int gy = gy0 + hyv[i], gx = gx0 + hxv[i];
                const bool ok = rel[i] >= 0 && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
                lds_dma16(dst + (uint32_t)(i * 1024 * NW), rs, ok ? base + rel[i] : (int)OOB, 0);
            }
        }
    };

    // uint8 frames: the next tile's halo bytes are fetched into registers where the DMA would be issued and written to the other halo
    // buffer after this tile's MFMAs (nobody reads that buffer between the two barriers around them)
    // two register sets: the bytes of tile t + 2G are requested at the top of tile t and written to LDS at the end of tile t + 1 -- a whole tile
    // period for the loads to land (requested and consumed inside ONE tile their ~2 us were exposed every tile: 5.5 us per tile, 2.7 TB/s)
    U8Halo<NTR> u8s[2];
    bf16_t* u8lut = reinterpret_cast<bf16_t*>(smem_raw + WBYTES + NBUF * HBYTES);       // 512 bytes behind the halo buffers (host adds them)
    if (U8) { u8_lut_init(u8lut, tid); __syncthreads(); }
    auto u8_load = [&](int tile, U8Halo<NTR>& u8h) {
        const int n = tile / tiles_img;
        const int tr = tile - n * tiles_img;
        const int ty = tr / tiles_x, tx = tr - ty * tiles_x;
        u8h.template load<NSLOT>(p.u8, n, p.H, p.W, ty * TH * ST + hy0, tx * TW * ST + hx0, wid, hyv, hxv, rel);
    };
    const int frow = lane & 15, g4 = lane >> 4;
    int cur = 0;
    // persistent walk: round i covers tiles [i*G, (i+1)*G); inside a round every XCD takes a contiguous run (shared halo rows hit L2)
    int tile = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    bool first = true;
    if (U8) {
        if (tile < ntiles) {
            u8_load(tile, u8s[0]);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); u8s[0].landed();
            u8s[0].template store<NSLOT>(smem_raw + WBYTES, u8lut, wid, lane);
        }
        if (tile + (int)gridDim.x < ntiles) u8_load(tile + gridDim.x, u8s[1]);
    } else if (tile < ntiles) issue_halo(0, tile);
    __syncthreads();                                                                   // filters visible
    // bias once per workgroup (a load inside the tile loop is a compiler-visible wait that also drains the next halo's transfers)
    f32x4 biasv[TI];
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        const int co = i * 16 + g4 * 4;
        biasv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if ((p.flags & DIN_CONV_BIAS) && co < p.Cout) biasv[i] = *reinterpret_cast<const f32x4*>(p.bias + co);
        asm volatile("" : "+v"(biasv[i]));                             // consumed HERE: the compiler's wait for the load stays out of the loop
    }
    auto tile_body = [&](auto PARC) {                                                  // PAR: which uint8 register set this tile FILLS
        constexpr int PAR = decltype(PARC)::value;
        // in-order completion: the halo transfers of this tile are older than the (always NST) stores of the previous tile when
        // double-buffered, so the stores may stay in flight; single-buffered the transfers are the youngest -> drain everything
        if (U8) {}                                                                     // (no transfers: the halo was written to LDS by the waves themselves)
        else if (NBUF == 2 && !first) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NST) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        first = false;
        __builtin_amdgcn_s_barrier();                                                  // halo(tile) landed; everyone left the previous tile
        asm volatile("" ::: "memory");
        const bool have_next = tile + (int)gridDim.x < ntiles;
        if (U8) { if (tile + 2 * (int)gridDim.x < ntiles) u8_load(tile + 2 * gridDim.x, u8s[PAR]); }
        else if (NBUF == 2 && have_next) issue_halo(cur ^ 1, tile + gridDim.x);
        const u32x4* Hl = reinterpret_cast<const u32x4*>(smem_raw + WBYTES + cur * HBYTES);
        // ---- dgrad epilogue operands (ReLU mask of the produced pixels, accumulate input): requested HERE, a whole MFMA phase before the
        //      epilogue uses them.  Fetched inside the store loop their HBM latency (~2 us) was exposed once per tile: the Conv2d_2a dgrad
        //      ran 1083 us inside the training step, 871 us with the early request (and 680 us with no mask at all).
        constexpr int NIT = (NPX / NPASS) * CPR / NTHREADS;
        const int n = tile / tiles_img;
        const int trm = tile - n * tiles_img;
        const int ty = trm / tiles_x, tx = trm - ty * tiles_x;
        __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(p.out) + (long long)n * oimg_bytes, 0, (int)oimg_bytes, 0x00020000);
        __amdgpu_buffer_rsrc_t rsM = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(reinterpret_cast<const char*>((p.flags & DIN_CONV_MASK) ? p.mask : p.out)) + (long long)n * mimg_bytes, 0,
            (p.flags & DIN_CONV_MASK) ? (int)mimg_bytes : 0, 0x00020000);
        auto out_pixel = [&](int ps, int it, int& opx, int& co) -> bool {              // pixel / channel chunk of store `it` of pass `ps`
            const int idx = it * NTHREADS + tid;
            const int srow = idx / CPR, c = idx - srow * CPR;
            const int w_ = srow / (JN * 16), rem = srow - w_ * (JN * 16);
            const int q = w_ * TJ + ps * JN + rem / 16;                                // segment of the tile
            const int gy = ty * TH + (q >> 1), gx = tx * TW + (q & 1) * 16 + (rem & 15);
            co = c * 8;
            opx = gy * p.OW + gx;
            return gy < p.OH && gx < p.OW && co < p.Cout;
        };
        u32x4 mkP[EPI ? NPASS : 1][EPI ? NIT : 1], oldP[EPI ? NPASS : 1][EPI ? NIT : 1];
        if (EPI && (p.flags & (DIN_CONV_MASK | DIN_CONV_ACCUM))) {
#pragma unroll
            for (int ps = 0; ps < (EPI ? NPASS : 1); ++ps)
#pragma unroll
                for (int it = 0; it < (EPI ? NIT : 1); ++it) {
                    int opx, co;
                    const bool ok = out_pixel(ps, it, opx, co);
                    mkP[ps][it] = u32x4{0u, 0u, 0u, 0u}; oldP[ps][it] = u32x4{0u, 0u, 0u, 0u};
                    if (p.flags & DIN_CONV_MASK)
                        mkP[ps][it] = __builtin_amdgcn_raw_buffer_load_b128(rsM, ok ? (opx * p.ldm + p.moff + co) * 2 : (int)OOB, 0, 0);
                    if (p.flags & DIN_CONV_ACCUM)
                        oldP[ps][it] = __builtin_amdgcn_raw_buffer_load_b128(rsO, ok ? (opx * p.ldo + p.cooff + co) * 2 : (int)OOB, 0, 0);
                }
        }

        f32x4 acc[TI][TJ];
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int ysgn = p.cy > 0 ? 1 : -1, xsgn = p.cx > 0 ? 1 : -1;
        const int yb = p.cy > 0 ? 0 : KH - 1, xb = p.cx > 0 ? 0 : KW - 1;
        if (CPP >= 4) {
#pragma unroll
            for (int tap = 0; tap < NTAPS; ++tap) {
                const int r = tap / KW, s2 = tap - r * KW;
                const int dy = yb + ysgn * r, dx = xb + xsgn * s2;
#pragma unroll
                for (int sl = 0; sl < SL; ++sl) {
                    u32x4 wf[TI], xf[TJ];
                    const int chunk = sl * 4 + g4;
#pragma unroll
                    for (int i = 0; i < TI; ++i) {
                        const int co = i * 16 + frow;
                        wf[i] = Wl[(tap * BN + co) * CPP + (chunk ^ swz(co))];
                    }
#pragma unroll
                    for (int j = 0; j < TJ; ++j) {
                        const int q = wid * TJ + j;                                     // 16-pixel segment of the tile
                        const int hp = ((q >> 1) * ST + dy) * HWW + ((q & 1) * 16 + frow) * ST + dx;
                        xf[j] = Hl[hp * CPP + (chunk ^ swz(hp))];
                    }
#pragma unroll
                    for (int i = 0; i < TI; ++i)
#pragma unroll
                        for (int j = 0; j < TJ; ++j) Mma<T>::run(wf[i], xf[j], acc[i][j]);
                }
            }
        } else {
#pragma unroll
            for (int sl = 0; sl < NSL; ++sl) {
                u32x4 wf[TI], xf[TJ];
                const int tap = min(sl * 4 + g4, NTAPS - 1);                           // surplus taps: finite data x zero filter
                const int r = tap / KW, s2 = tap - r * KW;
                const int dy = yb + ysgn * r, dx = xb + xsgn * s2;
#pragma unroll
                for (int i = 0; i < TI; ++i) wf[i] = Wl[(sl * BN + i * 16 + frow) * 4 + g4];
#pragma unroll
                for (int j = 0; j < TJ; ++j) {
                    const int q = wid * TJ + j;
                    xf[j] = Hl[((q >> 1) * ST + dy) * HWW + ((q & 1) * 16 + frow) * ST + dx];
                }
#pragma unroll
                for (int i = 0; i < TI; ++i)
#pragma unroll
                    for (int j = 0; j < TJ; ++j) Mma<T>::run(wf[i], xf[j], acc[i][j]);
            }
        }
        if (U8 && have_next) {
            // the bytes of tile + G were requested a tile ago; younger: the previous tile's stores and this tile's 3 NTR byte loads (if any)
            if (tile + 2 * (int)gridDim.x < ntiles) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(3 * NTR) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            u8s[PAR ^ 1].landed();
            u8s[PAR ^ 1].template store<NSLOT>(smem_raw + WBYTES + (cur ^ 1) * HBYTES, u8lut, wid, lane);
        }
        __syncthreads();                                                               // all waves done reading halo(cur)
        // ---- epilogue: stage through the consumed halo buffer, then 16-byte coalesced buffer stores (always NST per wave) -----
        unsigned char* stg = smem_raw + WBYTES + cur * HBYTES;
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                const f32x4 bv = biasv[i];
                const int co = i * 16 + g4 * 4;
#pragma unroll
                for (int j = ps * JN; j < (ps + 1) * JN; ++j) {
                    f32x4 v = acc[i][j] + bv;
                    if (p.flags & DIN_CONV_RELU) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                    }
                    const int srow = (wid * JN + (j - ps * JN)) * 16 + frow;             // staging row of this pixel
                    *reinterpret_cast<u32x2*>(stg + srow * CPITCH + co * 2) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
                }
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                int opx, co;
                const bool ok = out_pixel(ps, it, opx, co);
                const int idx = it * NTHREADS + tid;
                const int srow = idx / CPR, c = idx - srow * CPR;
                u32x4 v = *reinterpret_cast<const u32x4*>(stg + srow * CPITCH + c * 16);
                const int o = ok ? (opx * p.ldo + p.cooff + co) * 2 : (int)OOB;
                if (p.flags & (DIN_CONV_MASK | DIN_CONV_ACCUM)) {
                    u32x4 mk = {0u, 0u, 0u, 0u}, old = {0u, 0u, 0u, 0u};
                    if (EPI) { mk = mkP[EPI ? ps : 0][EPI ? it : 0]; old = oldP[EPI ? ps : 0][EPI ? it : 0]; }
                    else {
                        if (p.flags & DIN_CONV_MASK) mk = __builtin_amdgcn_raw_buffer_load_b128(rsM, ok ? (opx * p.ldm + p.moff + co) * 2 : (int)OOB, 0, 0);
                        if (p.flags & DIN_CONV_ACCUM) old = __builtin_amdgcn_raw_buffer_load_b128(rsO, o, 0, 0);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float lo = __uint_as_float(v[e] << 16), hi = __uint_as_float(v[e] & 0xffff0000u);
                        if (p.flags & DIN_CONV_MASK) {
                            if (!(__uint_as_float(mk[e] << 16) > 0.f)) lo = 0.f;
                            if (!(__uint_as_float(mk[e] & 0xffff0000u) > 0.f)) hi = 0.f;
                        }
                        if (p.flags & DIN_CONV_ACCUM) { lo += __uint_as_float(old[e] << 16); hi += __uint_as_float(old[e] & 0xffff0000u); }
                        v[e] = pack_bf16x2(lo, hi);
                    }
                }
                __builtin_amdgcn_raw_buffer_store_b128(v, rsO, o, 0, 0);                  // out-of-range offset -> dropped, still counted
            }
            if (ps + 1 < NPASS) __syncthreads();
        }
        if (NBUF == 2) cur ^= 1;
        else {
            __syncthreads();                                                            // staging buffer free again
            if (tile + (int)gridDim.x < ntiles) issue_halo(0, tile + gridDim.x);
        }
    };
    if constexpr (U8) {
        for (;;) {
            if (tile >= ntiles) break;
            tile_body(IcTag<0>{}); tile += gridDim.x;
            if (tile >= ntiles) break;
            tile_body(IcTag<1>{}); tile += gridDim.x;
        }
    } else {
        for (; tile < ntiles; tile += gridDim.x) tile_body(IcTag<0>{});
    }
#endif
}

// the instantiations, X(CPP, BN, NBUF, KH, KW, ST, U8, NW, EPI): the image layer (prepared tensor / raw uint8 frames), then the 64-byte and
// the 128-byte pixels of the 32- and 64-channel layers
#define DIN_CONV_SMALL_TABLE(X)                                                                                         \
    X(1, 32, 2, 3, 3, 2, 1, 4, 0) X(1, 32, 2, 3, 3, 2, 0, 4, 0)                                                         \
    X(4, 32, 2, 3, 3, 1, 0, 4, 1) X(4, 32, 2, 3, 3, 1, 0, 4, 0) X(4, 64, 2, 3, 3, 1, 0, 8, 0) X(4, 64, 2, 3, 3, 1, 0, 4, 0) \
    X(8, 32, 1, 3, 3, 1, 0, 4, 0) X(8, 32, 2, 3, 3, 1, 0, 8, 1) X(8, 32, 2, 3, 3, 1, 0, 8, 0) X(8, 32, 1, 3, 3, 1, 0, 8, 1) \
    X(8, 32, 1, 3, 3, 1, 0, 8, 0)

std::string small_kernel_name(const SmallVariant& s) {
    char line[96];
    snprintf(line, sizeof line, "conv_small_kernel<%d,%d,%d,3,3,%d,%d,%d,%d>", s.cpt, s.bn, s.nbuf, s.image ? 2 : 1, (int)(s.image && s.u8), s.waves, (int)s.epi);
    return line;
}

// the table row of a variant: launched on `st` when `k` is given, only looked up otherwise; a tuple without a row is an error
int small_row(const SmallVariant& s, const ConvK* k, hipStream_t st) {
    auto go = [&](auto kern) {
        if (!k) return DIN_OK;
        if (s.lds > 65536) raise_lds_limit(kern, s.lds);
        hipLaunchKernelGGL(kern, dim3(s.grid), dim3(64 * s.waves), s.lds, st, *k);
        return DIN_OK;
    };
#define DIN_ROW(CPP_, BN_, NBUF_, KH_, KW_, ST_, U8_, NW_, EPI_)                                                                           \
    if (s.cpt == CPP_ && s.bn == BN_ && s.nbuf == NBUF_ && (s.image ? 2 : 1) == ST_ && (s.image && s.u8) == (bool)U8_ && s.waves == NW_ && \
        s.epi == (bool)EPI_)                                                                                                               \
        return go(conv_small_kernel<CPP_, BN_, NBUF_, KH_, KW_, ST_, U8_, NW_, EPI_>);
    DIN_CONV_SMALL_TABLE(DIN_ROW)
#undef DIN_ROW
    DIN_FAIL(DIN_E_ARG, "conv_small: %s is not instantiated", small_kernel_name(s).c_str());
}

}  // namespace

namespace din_gather {

// Whether a launch (plan fields set: set_plan_fields) runs on conv_small_kernel, and on which variant with which LDS size and grid.
bool conv_small_variant(const ConvK& k, int dtype, SmallVariant& s) {
    const bool fast = k.divy == 1 && k.divx == 1, single = !k.remap && k.nsrc == 0 && k.csplit == 0;
    const bool common = conv_small_wanted() && dtype == DIN_BF16 && fast && single && k.splitk == 1 && k.kh == 3 && k.kw == 3 &&
                        k.Cout <= 64 && k.Cout % 8 == 0 && k.cooff % 8 == 0 && k.ldo % 8 == 0 && k.ldi % 8 == 0 && k.cioff % 8 == 0 &&
                        mask_views_aligned8(k) && views_below_2g(k) && k.out_sy == 0 && (int64_t)k.M >= 256 * 1024;
    // 32/64-channel 3x3 stride-1 layers (fwd and dgrad) ...
    const bool stem = common && (k.cpt == 4 || k.cpt == 8) && k.cpt * 8 == k.Cin && k.ay == 1 && k.ax == 1 &&
                      (k.cy == 1 || k.cy == -1) && (k.cx == 1 || k.cx == -1) && !(k.cpt == 8 && k.Cout > 32);
    // ... and the image layer: <= 8 (zero-padded) channels per pixel, stride 2, forward only
    const bool image = common && k.cpt == 1 && k.Cin <= 8 && k.ldi >= 8 && k.Cout <= 32 && k.ay == 2 && k.ax == 2 && k.cy == 1 && k.cx == 1 &&
                       k.wld >= 12;
    if (!stem && !image) return false;
    s.cpt = k.cpt; s.bn = k.Cout <= 32 ? 32 : 64; s.image = image; s.u8 = k.u8 != nullptr;
    const int st_ = image ? 2 : 1;
    const int hpx = (7 * st_ + 3) * (31 * st_ + 3);
    const int hbytes = (hpx * k.cpt * 16 + 1023) / 1024 * 1024;
    // 128-byte pixels (the 64-channel dgrad of Conv2d_2b): one halo buffer (80 KiB) or -- DIN_CONV_SMALL_NBUF8=2 -- two (124 KiB, the next
    // halo in flight under this tile's MFMAs like the 64-byte-pixel variants); one workgroup per CU either way
    const bool two8 = k.cpt == 8 && opt_int(DIN_OPT("DIN_CONV_SMALL_NBUF8"), 0) == 2;
    s.lds = (size_t)(image ? 3 * s.bn * 64 : 9 * s.bn * k.cpt * 16) + (size_t)((k.cpt == 8 && !two8) ? 1 : 2) * hbytes + (s.u8 ? 512 : 0);   // (+ the uint8 -> bf16 table)
    // the image layer's 42 KiB workgroups fit three to a CU: 768 persistent workgroups measured 690 -> 618 us on the 96 frames
    // (1024: no better, four do not fit); DIN_CONV_IMAGE_GRID overrides
    const int gv = opt_int(DIN_OPT("DIN_CONV_IMAGE_GRID"), 0);
    s.grid = image ? (gv > 0 ? gv : 768) : 512;
    // dgrad launches with a mask / accumulate operand: the variant that requests them a tile phase early (DIN_CONV_SMALL_EPI=0: in the store loop)
    const bool epi = (k.flags & (DIN_CONV_MASK | DIN_CONV_ACCUM)) && opt_int(DIN_OPT("DIN_CONV_SMALL_EPI"), 1) != 0;
    // the two 80 KiB variants (one workgroup per CU) run on eight waves; DIN_CONV_SMALL_WAVES=4 restores four
    // (64-byte pixels x 32 filters: eight waves measured slower, 706 -> 765 us)
    const bool w8 = !image && !(k.cpt == 4 && s.bn == 32) && opt_int(DIN_OPT("DIN_CONV_SMALL_WAVES"), 8) != 4;
    s.waves = w8 ? 8 : 4;
    s.nbuf = (k.cpt == 8 && !(two8 && w8)) ? 1 : 2;
    s.epi = epi && !image && ((k.cpt == 4 && s.bn == 32) || (k.cpt == 8 && w8));     // (the instantiations that exist)
    return true;
}

int launch_conv_small(const ConvK& k, const SmallVariant& s, hipStream_t st) { return small_row(s, &k, st); }

int append_conv_small_name(const SmallVariant& s, std::string& out) {
    if (int e = small_row(s, nullptr, nullptr)) return e;
    out += small_kernel_name(s); out += '\n';
    return DIN_OK;
}

}  // namespace din_gather
