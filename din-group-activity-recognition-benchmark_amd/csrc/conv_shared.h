// Shared between the forward / data-gradient sources (conv_igemm.hip, conv_halo.hip, conv_small.hip), conv_pack.hip and conv_wgrad.hip (weight
// gradient): the vector types, the workgroup size of the 256-thread kernels, the packing granularity and the geometry of a packed filter bank,
// the MFMA of one 16-byte chunk per storage type, the uint8 image-layer halo loader of the two stem kernels, and the host helpers the planners use.
#pragma once
#include "din_common.h"
#include <stdlib.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int NTHREADS = 256;
constexpr int KC = 8;        // 16-byte chunks per k-step of a packed filter bank (=> 128 B per tile row)

// ---- DIN_F32_BF16X3: fp32 operands multiplied as three bf16 parts each --------------------------------------------------------
// x = x0 + x1 + x2 exactly, 8 + 8 + 8 significand bits: x0 = the top 16 bits of x (TRUNCATED, so the high part of a value near FLT_MAX
// stays finite), x1 = the remainder rounded to nearest bf16, x2 = what is left (at most 8 significant bits: exact); both subtractions are
// exact.  Rounding the MIDDLE part to nearest instead of truncating it again halves the dropped cross terms a1 b2 + a2 b1 and makes them
// unbiased: with two truncations every part has the sign of x and the dropped terms add up one-sidedly -- tools/split_bf16_sim.py measures
// rms(err) 1.17x an fp32-accumulated exact product at K = 64 that way, 0.89x this way.  The parts come back as fp32 bit patterns whose
// bf16 half is the top one (the low halves are zero).
__device__ __forceinline__ void split_bf16x3(uint32_t x, uint32_t& x0, uint32_t& x1, uint32_t& x2) {
    x0 = x & 0xffff0000u;
    const float r1 = __uint_as_float(x) - __uint_as_float(x0);
    x1 = (uint32_t)f32_to_bf16(r1) << 16;
    x2 = __float_as_uint(r1 - __uint_as_float(x1));
}
// one 32-bit MFMA operand word = two bf16 k-slots: the top half of `hi` above the top half of `lo` (v_perm_b32)
__device__ __forceinline__ uint32_t bf16_halves(uint32_t hi, uint32_t lo) { return __builtin_amdgcn_perm(hi, lo, 0x07060302u); }
// c += A * B over the lane's 4 fp32 k-values of each operand (a: the MFMA's i side, b: its j side), as the six leading cross products of
// the parts in three v_mfma_f32_16x16x32_bf16: the lane's 8 k-slots hold two parts of its 4 values, word e = (slot 2e, slot 2e + 1):
//   [a2 | a0] x [b0 | b2]  = a2 b0 + a0 b2        [a1 | a0] x [b1 | b1]  = a1 b1 + a0 b1        [a1 | a0] x [b0 | b0]  = a1 b0 + a0 b0
// (smallest terms first; a1 b2, a2 b1, a2 b2 <= 2^-23 of a product are dropped).  3 x 16 matrix-pipe cycles against the 4 x 32 of four
// v_mfma_f32_16x16x4_f32, for 8-9 VALU instructions per fp32 value (measured: profiles/fp32_split_step_time.txt).
__device__ __forceinline__ void mma_f32_bf16x3(const u32x4& a, const u32x4& b, f32x4& c) {
    u32x4 a01, a02, b00, b11, b20;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uint32_t p0, p1, p2, q0, q1, q2;
        split_bf16x3(a[e], p0, p1, p2);
        split_bf16x3(b[e], q0, q1, q2);
        a01[e] = bf16_halves(p0, p1); a02[e] = bf16_halves(p0, p2);
        b00[e] = bf16_halves(q0, q0); b11[e] = bf16_halves(q1, q1); b20[e] = bf16_halves(q2, q0);
    }
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a02), __builtin_bit_cast(bf16x8, b20), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a01), __builtin_bit_cast(bf16x8, b11), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a01), __builtin_bit_cast(bf16x8, b00), c, 0, 0, 0);
}

// one 16-byte chunk of each operand into the MFMA, per storage type (conv_igemm.hip: the header comment)
template <typename T> struct Mma;
template <> struct Mma<float> {
    __device__ static void run(const u32x4& a, const u32x4& b, f32x4& c) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[j]), __uint_as_float(b[j]), c, 0, 0, 0);
    }
};
// fp32 chunks multiplied as three bf16 parts.  The split is formed per fragment read: inside the unrolled fragment loops of a
// k-step the compiler forms each fragment's parts once and reuses them across the (i, j) pairs.
template <> struct Mma<f32x3_t> {
    __device__ static void run(const u32x4& a, const u32x4& b, f32x4& c) { mma_f32_bf16x3(a, b, c); }
};
template <> struct Mma<bf16_t> {
    __device__ static void run(const u32x4& a, const u32x4& b, f32x4& c) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};

// ---- image layer fed from raw uint8 frames (din_conv_desc::in_u8): the halo pixels of a tile are fetched as bytes from the three colour
//      planes, normalised exactly like utils.prep_images ((x / 255 - 0.5) * 2: three separately rounded fp32 operations, utils.py:8-19),
//      rounded to bf16 and written to the LDS position the LDS-DMA of a prepared NHWC tensor would have filled (16 bytes per pixel:
//      r, g, b and five zero channels; pixels outside the image are zero).  Lane-linear: halo pixel id = (wave + 4 i) * 64 + lane.
__device__ __forceinline__ float prep_u8(uint32_t v) {
    float y = __fdiv_rn((float)v, 255.0f);
    y = __fsub_rn(y, 0.5f);
    return __fmul_rn(y, 2.0f);
}
__device__ __forceinline__ void u8_lut_init(bf16_t* lut, int tid) {          // NTHREADS == 256: one entry per thread
    lut[tid] = (bf16_t)(pack_bf16x2(prep_u8((uint32_t)tid), 0.f) & 0xffffu);
}
template <int NTR>
struct U8Halo {
    // the three bytes of a pixel stay in separate registers until store(): nothing consumes them at load time, so the loads stay in flight
    // under the tile's MFMAs instead of being waited for where they are issued
    uint32_t r[NTR], g[NTR], b[NTR];
    uint32_t valid;                                      // bit i: pixel i lies inside the image
    // hyv / hxv: the lane's halo coordinates per transfer (the kernels' tile-independent DMA plans); inside[i]: the id is a halo pixel
    template <int NSLOT>
    __device__ __forceinline__ void load(const unsigned char* __restrict__ img, int n, int H, int W, int gy0, int gx0, int wid,
                                         const short (&hyv)[NTR], const short (&hxv)[NTR], const int (&inside)[NTR]) {
        // every lane ALWAYS loads (coordinates clamped into the image, validity kept as a bit): a load inside `if (inside)` merges with the zero
        // of the other path at the end of the branch, and the compiler waits for it right there -- five exposed memory latencies per tile
        // (vmcnt(2) / (1) / (0) after every pixel in the ISA; the image layer ran 5.5 us per tile = 2.7 TB/s because of it)
        const int64_t plane = (int64_t)H * W;
        const unsigned char* base = img + (int64_t)n * 3 * plane;
        valid = 0u;
#pragma unroll
        for (int i = 0; i < NTR; ++i) {
            const int gy = gy0 + hyv[i], gx = gx0 + hxv[i];
            const bool ok = wid + 4 * i < NSLOT && inside[i] >= 0 && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const unsigned char* q = base + (int64_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1);
            // untracked loads (inline asm): the compiler would zero-extend the bytes -- i.e. wait for them -- right here; the caller waits by
            // count (s_waitcnt vmcnt) before store() and calls landed()
            asm volatile("global_load_ubyte %0, %1, off" : "=&v"(r[i]) : "v"(q) : "memory");
            asm volatile("global_load_ubyte %0, %1, off" : "=&v"(g[i]) : "v"(q + plane) : "memory");
            asm volatile("global_load_ubyte %0, %1, off" : "=&v"(b[i]) : "v"(q + 2 * plane) : "memory");
            valid |= (ok ? 1u : 0u) << i;
        }
    }
    __device__ __forceinline__ void landed() {                       // after the caller's s_waitcnt: ties the registers to this point
#pragma unroll
        for (int i = 0; i < NTR; ++i) { asm volatile("" : "+v"(r[i])); asm volatile("" : "+v"(g[i])); asm volatile("" : "+v"(b[i])); }
    }
    // lut: the 256 normalised bf16 values (prep_u8 of every byte, built once per workgroup by u8_lut_init) -- three LDS reads per pixel
    // instead of three fp32 divisions
    template <int NSLOT>
    __device__ __forceinline__ void store(unsigned char* lds_buf, const bf16_t* lut, int wid, int lane) const {   // lds_buf: the halo buffer
#pragma unroll
        for (int i = 0; i < NTR; ++i) {
            if (wid + 4 * i < NSLOT) {
                u32x4 v = {0u, 0u, 0u, 0u};
                if ((valid >> i) & 1u) {
                    v[0] = (uint32_t)lut[r[i]] | ((uint32_t)lut[g[i]] << 16);
                    v[1] = (uint32_t)lut[b[i]];
                }
                *reinterpret_cast<u32x4*>(lds_buf + ((wid + 4 * i) * 64 + lane) * 16) = v;
            }
        }
    }
};

// ---- host side ---------------------------------------------------------------------------------------
inline int epc_of(int dtype) { return dtype == DIN_F32 ? 4 : 8; }
inline int pad_to(int v, int m) { return (v + m - 1) / m * m; }
inline int opt_int(const char* v, int dflt) { return v ? atoi(v) : dflt; }
// DIN_F32_BF16X3 is DIN_F32 in everything but the MMA.  Every contraction entry point starts with `const SplitDesc sd(d);`: from there on
// `d` is the same descriptor with DIN_F32 (plan, tile choice, workspace, packing and every byte-size rule are that descriptor's), and
// sd.split travels to the launch (ConvK::mma, plan_wgrad's second argument) to pick the kernels that multiply in three bf16 parts.
inline int storage_dtype(int dtype) { return dtype == DIN_F32_BF16X3 ? DIN_F32 : dtype; }
struct SplitDesc {
    din_conv_desc copy;
    bool split = false;
    explicit SplitDesc(const din_conv_desc*& d) {
        if (d && d->dtype == DIN_F32_BF16X3) { copy = *d; copy.dtype = DIN_F32; d = &copy; split = true; }
    }
};
// The packed filter bank of a descriptor (dtype: the storage type), forward (transposed = 0: row = co, k = (r, s, ci)) or data-gradient
// orientation (1: row = ci, k = (r, s, co)): cred reduction channels per tap, padded to whole chunks (inner_pad elements = cpt chunks), nk
// k-steps of KC chunks = kelems elements per row, cprod rows padded to the widest filter tile (rows_pad).
struct PackGeom { int cred, cprod, inner_pad, cpt, nk, kelems, rows_pad; };
inline PackGeom pack_geom(const din_conv_desc* d, int transposed) {
    const int epc = epc_of(d->dtype);
    PackGeom g;
    g.cred = transposed ? d->cout : d->cin; g.cprod = transposed ? d->cin : d->cout;
    g.inner_pad = pad_to(g.cred, epc); g.cpt = g.inner_pad / epc;
    g.nk = (d->kh * d->kw * g.cpt + KC - 1) / KC; g.kelems = g.nk * KC * epc;
    g.rows_pad = pad_to(g.cprod, 256);
    return g;
}
// stem layers on conv_small_kernel / conv_wgrad_small_kernel (DIN_CONV_SMALL=0: off); din_conv_accepts_u8 answers from the same switch
inline bool conv_small_wanted() { return opt_int(DIN_OPT("DIN_CONV_SMALL"), 1) != 0; }

// hipFuncSetAttribute is a slow host call: raise a kernel's dynamic-LDS limit once per (thread, kernel), not per launch
template <typename K>
inline void raise_lds_limit(K kern, size_t lds) { din_raise_lds(reinterpret_cast<const void*>(kern), lds); }

}  // namespace

namespace din_conv {
int check_desc(const din_conv_desc* d);          // conv_igemm.hip: the descriptor rules every conv entry point starts with
}
