// Shared between the filter-resident halo kernels (conv_halo_rf.hip: 3x3, conv_halo_rf5.hip: 5x5): the inline-asm primitives that fix
// where every operand lives, the 8 x 32 tile and its work items, the pieces of the epilogue, and the host side that does not depend on the
// walk -- the planner's common half and the bodies of the four entry points of a family.  Each family keeps its kernel, its halo plan,
// its LDS size, its instantiation table and its measured planner rule.
// A device piece lives here only if both families compile to the instruction streams they had with the piece written out in the kernel:
// the epilogue's store, the bias staging and mask_one did not (or differ between the families) and stay in the kernels.
#pragma once
#include "din_common.h"
#include "conv_gather.h"
#include "conv_shared.h"
#include <stdlib.h>
#include <string>
#include <type_traits>

namespace din_rf {

using din_gather::ConvK;

constexpr int TH = 8, TW = 32;                                                    // pixels of a tile: four rows per pixel half, two fragments per row
constexpr unsigned OOB = 0x80000000u;                                             // a buffer offset out of range of every view (< 2 GiB: views_below_2g)

template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}
template <int OFF>
__device__ __forceinline__ void read(u32x4& dst, uint32_t addr) {
    static_assert(OFF >= 0 && OFF < 65536, "ds_read offset field");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
template <bool ACC>
__device__ __forceinline__ void pin(u32x4& x) {                  // the value lives in an accumulation (ACC) or an architectural register from here on
    if constexpr (ACC) asm volatile("" : "+a"(x));
    else asm volatile("" : "+v"(x));
}
// c (+)= a x b.  Inline asm, with the register file of every operand chosen here (ACC: the filter fragment sits in an accumulation
// register): through the builtin the allocator keeps every fragment it can in architectural registers and copies the others there in
// front of their MFMA (904 v_accvgpr_read per tile in the first build of the 96 -> 96 form).  FIRST: the tile's first k-step, C = 0.
template <bool ACC, bool FIRST>
__device__ __forceinline__ void mfma(f32x4& c, const u32x4& a, const u32x4& b) {
    if constexpr (FIRST) {
        if constexpr (ACC) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&a"(c) : "a"(a), "v"(b));
        else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&a"(c) : "v"(a), "v"(b));
    } else {
        if constexpr (ACC) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "a"(a), "v"(b));
        else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
    }
}
template <int N>
__device__ __forceinline__ void wait(u32x4& x) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(x) : "n"(N)); }

// a work item: tile (ty, tx) of image n; items are numbered image-major over tiles_img = tiles_y * tiles_x tiles
struct Item { int n, ty, tx; };
__device__ __forceinline__ Item decode_item(int item, int tiles_img, int tiles_x) {
    Item it;
    it.n = item / tiles_img;
    const int tr = item - it.n * tiles_img;
    it.ty = tr / tiles_x; it.tx = tr - it.ty * tiles_x;
    return it;
}

// ---- the epilogue's pieces: a lane holds four consecutive channels of a pixel as f32x4, their bf16 operands as u32x2
// ReLU-backward mask: v[e] = 0 unless bf16 e of mk is > 0
__device__ __forceinline__ void mask4(f32x4& v, const u32x2& mk) {
    if (!(__uint_as_float(mk[0] << 16) > 0.f)) v[0] = 0.f;
    if (!(__uint_as_float(mk[0] & 0xffff0000u) > 0.f)) v[1] = 0.f;
    if (!(__uint_as_float(mk[1] << 16) > 0.f)) v[2] = 0.f;
    if (!(__uint_as_float(mk[1] & 0xffff0000u) > 0.f)) v[3] = 0.f;
}
// ACCUM: v + the four bf16 of old.  (By value on purpose: with `v` taken by reference the compiler schedules every kernel differently.)
__device__ __forceinline__ f32x4 accum4(f32x4 v, u32x2 old) {
    v[0] += __uint_as_float(old[0] << 16); v[1] += __uint_as_float(old[0] & 0xffff0000u);
    v[2] += __uint_as_float(old[1] << 16); v[3] += __uint_as_float(old[1] & 0xffff0000u);
    return v;
}
// byte offset of channels co .. co + 3 of the pixel at pxo, for the accumulate load and the store (out of range: pxo has bit 31 set and
// stays >= 2^31 as an unsigned offset; Cout % 8 == 0: a piece is whole or absent).  The store itself stays in the kernels: as a function
// of any signature it changed the instruction order of the 3x3 kernels (profiles/halo_rf_refactor.txt).
__device__ __forceinline__ int piece_off(int pxo, int co, int Cout) { return co < Cout ? pxo + co * 2 : (int)OOB; }

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// padded-area waste of the 8 x 32 tile grid must stay moderate (plan_halo's rule)
static inline bool tile_waste_ok(int oh, int ow) {
    const int64_t padded = (int64_t)((oh + TH - 1) / TH * TH) * ((ow + TW - 1) / TW * TW);
    return padded * 100 <= (int64_t)oh * ow * 118;
}

// What the families' planners share, for the launch `which` (0 forward, 1 data gradient) of a descriptor: bf16, taps_1d x taps_1d, stride
// 1, dilation 1, reduction and produced channels in 40 .. cmax and multiples of 8, the flags of the direction, views as conv_halo_kernel
// takes them except the mask view (whole 16-byte chunks: it travels by LDS-DMA), DIN_CONV_HALO not 0; then the launch's geometry in k.
// Reads no pointer.
static inline bool plan_common(const din_conv_desc* d, int which, int flags, int ldm, int moff, int taps_1d, int cmax, ConvK& k) {
    if (!d || (which != 0 && which != 1) || d->dtype != DIN_BF16 || d->in_u8) return false;
    if (d->nb <= 0 || d->h <= 0 || d->w <= 0 || d->cin <= 0 || d->cout <= 0) return false;
    if (d->kh != taps_1d || d->kw != taps_1d || d->sh != 1 || d->sw != 1 || d->dh != 1 || d->dw != 1) return false;
    if (d->oh != d->h + 2 * d->ph - (taps_1d - 1) || d->ow != d->w + 2 * d->pw - (taps_1d - 1) || d->oh <= 0 || d->ow <= 0) return false;
    if ((int64_t)d->nb * d->h * d->w >= (1ll << 31) || (int64_t)d->nb * d->oh * d->ow >= (1ll << 31)) return false;
    const int cred = which ? d->cout : d->cin, cprod = which ? d->cin : d->cout;
    if (cred % 8 != 0 || cprod % 8 != 0 || cred < 40 || cred > cmax || cprod < 40 || cprod > cmax) return false;
    if (d->ldi % 8 != 0 || d->cioff % 8 != 0 || d->ldi < d->cioff + d->cin || d->ldo % 4 != 0 || d->cooff % 4 != 0 || d->ldo < d->cooff + d->cout) return false;
    if (which == 0 && (flags & ~(DIN_CONV_BIAS | DIN_CONV_RELU))) return false;
    if (which == 1) {
        if (flags & ~(DIN_CONV_MASK | DIN_CONV_ACCUM)) return false;
        if (d->ldo % 8 != 0 || d->cooff % 8 != 0) return false;                  // the gradient operand is read in whole chunks
        if ((flags & DIN_CONV_MASK) && (ldm % 8 != 0 || moff % 8 != 0 || moff < 0 || ldm < moff + cprod)) return false;
    }
    const char* hv = DIN_OPT("DIN_CONV_HALO");
    if (hv && atoi(hv) == 0) return false;
    k = ConvK{};
    k.NB = d->nb; k.kh = k.kw = taps_1d;
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
    k.cpt = bank.cpt; k.Q = taps_1d * taps_1d * bank.cpt; k.nk = bank.nk; k.wld = bank.nk * KC;
    k.flags = flags; k.ldm = (flags & DIN_CONV_MASK) ? ldm : 0; k.moff = (flags & DIN_CONV_MASK) ? moff : 0;
    k.splitk = 1; k.ks_per_split = k.nk; k.n_co_tiles = 1;
    return din_gather::views_below_2g(k);
}

// ---- the four entry points of a family F: F::Inst (its instantiation tuple), F::plan (eligibility, geometry and instantiation of a
// launch), F::row (the table row of an instantiation: launched when a ConvK is given, only looked up otherwise), F::name (the kernel as
// rocprofv3 prints it) and F::prefix (what its messages begin with)
template <class F>
int eligible(const din_conv_desc* d, int which, int flags, int ldm, int moff) {
    ConvK k; typename F::Inst r;
    return F::plan(d, which, flags, ldm, moff, k, r) && F::row(r, nullptr, nullptr) == DIN_OK ? 1 : 0;
}

template <class F>
int fwd(const din_conv_desc* d, const void* in, const void* wpk, const float* bias, void* out, int flags, void* stream) {
    const std::string who = std::string(F::prefix) + "_fwd";
    if (int e = din_conv::check_desc(d)) return e;
    DIN_REQUIRE(in && wpk && out, "%s: null pointer", who.c_str());
    DIN_REQUIRE(!(flags & DIN_CONV_BIAS) || bias, "%s: BIAS flag without bias", who.c_str());
    ConvK k; typename F::Inst r;
    DIN_REQUIRE(F::plan(d, 0, flags, 0, 0, k, r), "%s: not eligible (ask din_%s_eligible)", who.c_str(), F::prefix);
    k.in = in; k.w = wpk; k.out = out; k.bias = bias;
    if (int e = F::row(r, &k, as_stream(stream))) return e;
    DIN_CHECK_LAUNCH(who.c_str());
    return DIN_OK;
}

template <class F>
int dgrad(const din_conv_desc* d, const void* dout, const void* wpk_t, void* din_, const void* mask, int ldm, int moff, int flags, void* stream) {
    const std::string who = std::string(F::prefix) + "_dgrad";
    if (int e = din_conv::check_desc(d)) return e;
    DIN_REQUIRE(dout && wpk_t && din_, "%s: null pointer", who.c_str());
    DIN_REQUIRE(!(flags & DIN_CONV_MASK) || mask, "%s: MASK flag without mask", who.c_str());
    ConvK k; typename F::Inst r;
    DIN_REQUIRE(F::plan(d, 1, flags, ldm, moff, k, r), "%s: not eligible (ask din_%s_eligible)", who.c_str(), F::prefix);
    k.in = dout; k.w = wpk_t; k.out = din_; k.mask = mask;
    if (int e = F::row(r, &k, as_stream(stream))) return e;
    DIN_CHECK_LAUNCH(who.c_str());
    return DIN_OK;
}

template <class F>
int kernel_names(const din_conv_desc* d, int which, int flags, int ldm, int moff, char* buf, int buf_bytes) {
    if (int e = din_conv::check_desc(d)) return e;
    DIN_REQUIRE(buf_bytes >= 0 && (buf || buf_bytes == 0), "%s_kernel_names: bad argument", F::prefix);
    ConvK k; typename F::Inst r;
    DIN_REQUIRE(F::plan(d, which, flags, ldm, moff, k, r), "%s_kernel_names: not eligible (ask din_%s_eligible)", F::prefix, F::prefix);
    if (int e = F::row(r, nullptr, nullptr)) return e;
    return copy_names(F::name(r) + "\n", buf, buf_bytes);
}

}  // namespace din_rf
