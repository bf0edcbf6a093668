/* din_hip.h -- C ABI of libdin_hip.so: the MI355X (gfx950) kernels behind the DIN stage-2 hot path.
 *
 * The reference (JacobYuan7/DIN-Group-Activity-Recognition-Benchmark) is pure Python; its only native
 * boundary is the third-party `roi_align` torch extension.  This header therefore DEFINES the native
 * boundary a maintainer would bind (ctypes stub shown in INTEGRATION.md); each entry cites the reference
 * interface (file:line, relative to the reference root) whose arithmetic it replaces.
 *
 * Conventions
 *  - plain C types only; every pointer is a DEVICE pointer owned by the caller (PyTorch-ROCm allocates);
 *    the library never allocates, never frees, never synchronises, never throws.
 *  - every function returns 0 on success or a negative DIN_E_* code; din_last_error_string() gives the
 *    thread-local message.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *  - activations are NHWC ("pixel-major"): element (n,y,x,c) of a tensor with pixel stride `ld` and
 *    channel offset `coff` lives at ((n*H+y)*W+x)*ld + coff + c.  ld/coff let several producers write
 *    disjoint channel ranges of one buffer (torch.cat(dim=1) at infer_model.py:172 and in the Inception
 *    blocks costs nothing).
 *  - dtype: DIN_F32 (parity mode, fp32 storage + fp32 MFMA accumulate) or DIN_BF16 (throughput mode:
 *    bf16 storage, fp32 MFMA accumulate).  Everything after RoIAlign is always fp32.
 *  - stateless and re-entrant: safe from autograd worker threads, concurrently on different streams.  The
 *    library never reads the process environment: kernel-selection switches used by the tests and the
 *    tuning tools are process-wide OPTIONS set through din_set_option (unset = the shipped choice).
 */
#ifndef DIN_HIP_H
#define DIN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIN_ABI_VERSION 9   /* 9: din_conv_wgrad_group (the weight gradients of several layers in one launch); din_basenet_head_fwd / _bwd were added later as a purely additive change (no existing signature changed), so the version stays 9.   8: din_set_option / din_get_option replace every getenv() of the library (tests select kernels through the ABI; a stray environment variable can no longer change a launch).   7: din_conv_dgrad_x (a strided dgrad that carries the 1x1 / stride-1 dgrad of a sibling conv reading the same view).   6: batch-statistics BatchNorm is deterministic: din_bn_stats / din_bn_bwd_stats write per-workgroup fp64 slabs into a workspace (din_bn_workspace), din_bn_finalize / din_bn_reduce add them in slab order -- no atomics, nothing for the caller to zero.   5: dropout seeds take an optional device-side offset (din_layernorm_*, din_act_dropout_*), din_counter_add, din_conv1x1_wgrad_multi.   2: din_walk_* take plain / clamp / n_per_clip; + bn, mask_actors.  3: din_roi_align_* take the box grid and a crop channel range.  4: din_conv_desc.in_u8, context-encoding entry points */

enum {
    DIN_F32 = 0, DIN_BF16 = 1,
    /* fp32 STORAGE, three-part bf16 MFMA COMPUTE (an additive value: no entry point, no signature changed).  Accepted wherever a
     * contraction takes DIN_F32 -- din_conv_fwd / _fwd2 / _dgrad / _dgrad_x, din_conv1x1_dgrad_multi, din_conv_wgrad / _wgrad_group,
     * din_conv1x1_wgrad_multi, the pack / packed_elems / workspace_bytes calls, din_conv_kernel_tile / _variant / _names,
     * din_conv_accepts_u8 (answers 0) -- and means: every tensor, the packed filter bank (bit-identical), the plan, the tile, the workspace
     * and every byte-size rule are those of the same descriptor with DIN_F32; only the multiply differs.  Each fp32 operand is split into
     * three bf16 parts, x = x0 + x1 + x2 exactly (8 + 8 + 8 significand bits: x0 = the top 16 bits, TRUNCATED so that it stays finite near
     * FLT_MAX; x1 = the remainder rounded to nearest, which keeps the dropped terms unbiased; x2 = what is left), and the six leading cross products
     * a0b0, a1b0, a0b1, a1b1, a0b2, a2b0 are accumulated in fp32 by three v_mfma_f32_16x16x32_bf16 in place of four
     * v_mfma_f32_16x16x4_f32; the dropped terms are <= 2^-23 of a product, so the result has fp32 accuracy (the tests hold it to the
     * fp32 bars unchanged).  din_conv_kernel_names spells these kernels with their own type token (conv_gather_fast_kernel<f32x3,...>,
     * conv_wgrad_f32x3_kernel).  Limits of the mode:
     *   - a lower part that falls below the bf16 normal range is lost: in practice values with |x| below about 2^-100 keep fewer than
     *     24 bits (their high part is always kept);
     *   - a non-finite operand reaches the result through its high part only: NaN stays NaN, and +-Inf gives a non-finite result that
     *     may be NaN where exact fp32 gives Inf (the lower parts of Inf are Inf - Inf).
     * Entry points that only move or normalise data (bn, pool, roi, cast, prep, colsum) keep taking the storage type, DIN_F32.          */
    DIN_F32_BF16X3 = 2
};

enum {
    DIN_OK = 0,
    DIN_E_ARG = -1,      /* bad argument (shape, alignment, null pointer)            */
    DIN_E_LAUNCH = -2,   /* hipLaunch / hipGetLastError failure                       */
    DIN_E_WORKSPACE = -3,/* caller-provided workspace too small                       */
    DIN_E_UNSUPPORTED = -4
};

int din_abi_version(void);
const char* din_last_error_string(void);
/* name of the device code object's target ("gfx950"); lets the host fail loudly on a wrong build */
const char* din_build_arch(void);
/* Process-wide tuning / test options ("DIN_CONV_HALO" = "2", ...; value NULL = unset).  They select between kernels that
 * compute the same result (tests cover every instantiation through them; tools/ A/B them); production code never sets any.
 * Thread-safe; a launch reads each option it consults exactly once.  The reference has no counterpart (its only knobs are
 * the Config fields, config.py:10-104, which stay in the Python layer). */
int din_set_option(const char* name, const char* value);
/* copies the current value into buf (empty string when unset); returns 1 if set, 0 if unset, negative on error */
int din_get_option(const char* name, char* buf, int buf_bytes);

/* ------------------------------------------------------------------------------------------------
 * Row P  prep_images  (utils.py:8-19): y = ((x/255) - 0.5) * 2, same three fp32 roundings.
 * ---------------------------------------------------------------------------------------------- */
/* NCHW fp32 -> NCHW fp32, API-parity form of utils.prep_images */
int din_prep_images_f32(const float* in, float* out, int64_t n, void* stream);
/* fused loader for the backbone: NCHW (uint8 or fp32, values 0..255) -> normalised NHWC with the channel
 * dimension zero-padded to `cpad` (4 for DIN_F32, 8 for DIN_BF16) so conv1 reads 16-byte pixels.      */
int din_prep_images_nhwc(const void* in, int in_is_u8, void* out, int out_dtype,
                         int nb, int h, int w, int cpad, void* stream);
/* backward of the loader is never needed (images carry no gradient: train_net_dynamic.py:175). */

/* ------------------------------------------------------------------------------------------------
 * Rows V, I, E, L, D1  dense contractions: implicit-GEMM convolution on MFMA.
 * Replaces torch.nn.Conv2d / nn.Linear arithmetic reached from backbone/backbone.py:44-99,
 * infer_model.py:184 (fc_emb_1), :190 (point_conv), :226 (fc_activities),
 * dynamic_infer_module.py:149 (hidden_weight), :191 (p_conv), :195 (scale_conv).
 * A Linear layer is the 1x1 case with NB=1, H=1, W=rows.
 * ---------------------------------------------------------------------------------------------- */
typedef struct din_conv_desc {
    int32_t nb, h, w, cin;          /* input  tensor [nb,h,w,cin], pixel stride ldi, channel offset cioff   */
    int32_t oh, ow, cout;           /* output tensor [nb,oh,ow,cout], pixel stride ldo, channel offset cooff */
    int32_t kh, kw, sh, sw, ph, pw, dh, dw;
    int32_t ldi, cioff, ldo, cooff;
    int32_t dtype;                  /* DIN_F32 / DIN_BF16 : storage type of in, out and packed weights; DIN_F32_BF16X3: DIN_F32
                                       storage, three-part bf16 multiply (see the enum above)                  */
    int32_t in_u8;                  /* 1: `in` is the raw uint8 clip batch [nb][3][h][w] (volleyball.py:223-275 frames before
                                       utils.prep_images) and the image layer normalises on load -- (x/255 - 0.5)*2 in the reference's
                                       three fp32 roundings, utils.py:8-19 -- instead of reading a prepared NHWC tensor; ldi / cioff are
                                       ignored.  Only din_conv_fwd / din_conv_wgrad, only where din_conv_accepts_u8() says so. */
} din_conv_desc;

enum {
    DIN_CONV_BIAS = 1,   /* out += bias[cout]  (fp32 vector)                                    */
    DIN_CONV_RELU = 2,   /* out = max(out, 0)                                                    */
    DIN_CONV_ACCUM = 4,  /* dgrad only: out += result (several consumers of one tensor)          */
    DIN_CONV_MASK = 8    /* dgrad only: result *= (mask > 0)  -- fused ReLU backward, mask has the
                            layout of the dgrad output (pixel stride ldm, channel offset moff)    */
};

/* number of elements (of desc->dtype) of the packed filter bank for fwd (transposed=0) / dgrad (=1) */
int64_t din_conv_packed_elems(const din_conv_desc* d, int transposed);
/* w: reference layout [cout][cin][kh][kw] fp32.  scale (nullable, [cout] fp32) is folded into the filters
 * (BatchNorm-eval: backbone.py BasicConv2d).  transposed=0 -> [cout_pad][(r,s,ci)], =1 -> [cin_pad][(r,s,co)] */
int din_conv_pack_weights(const din_conv_desc* d, const float* w, const float* scale, void* wpk,
                          int transposed, void* stream);
/* All filter banks of a backbone in ONE launch.  din_conv_pack_desc fills one table entry on the host (same layout rules as
 * din_conv_pack_weights); the caller uploads the table once and then calls din_conv_pack_multi every step with, per workgroup, the
 * bank it packs (layer_of) and which chunk_elems-sized chunk of it (chunk_index).  All three arrays live on the device. */
typedef struct din_pack_desc {
    uint64_t w, scale, out;          /* device addresses: fp32 [cout][cin][kh][kw] filters, fp32 [cout] scale (0: none), packed bank */
    int32_t cout, cin, kh, kw;
    int32_t rows, rows_pad, inner, inner_pad, kelems, transposed, dtype;
    int32_t reserved;
} din_pack_desc;
int din_conv_pack_desc(const din_conv_desc* d, const float* w, const float* scale, void* wpk, int transposed, din_pack_desc* out);
int din_conv_pack_multi(const din_pack_desc* table, const int32_t* layer_of, const int32_t* chunk_index, int nblocks,
                        int chunk_elems, void* stream);
/* Forward conv with TWO destinations: produced channels [0, csplit) go to `out` (desc->ldo / desc->cooff), channels [csplit, desc->cout) to
 * `out2` (pixel stride ldo2, channel offset cooff2).  For sibling convs that read the same tensor (torchvision InceptionA: branch1x1,
 * branch5x5_1, branch3x3dbl_1 -- backbone.py MyInception_v3 via torchvision inception.py InceptionA.forward): one launch over the
 * concatenated filter bank reads the input once and runs on a wide tile.  wpk = the banks of the siblings packed row after row (same cin,
 * kh, kw); bias = their shifts concatenated.  craw > 0: channels >= craw are stored raw (no bias, no ReLU) -- the branch_pool conv whose
 * bias + ReLU follow its average pool.  Not available for shapes that need split-K (returns DIN_E_ARG: launch them separately). */
int din_conv_fwd2(const din_conv_desc* d, const void* in, const void* wpk, const float* bias, void* out, void* out2, int ldo2, int cooff2,
                  int csplit, int craw, int flags, void* workspace, int64_t workspace_bytes, void* stream);
/* which tile variant the planner picks (which: 0 fwd, 1 dgrad -> pixels x filters of conv_gather_*_kernel; 2 wgrad -> filter rows x
 * k columns of conv_wgrad_*_kernel, bn = 1000 + k columns for conv_wgrad_ring_kernel; bm = 0 -> the stationary-filter stem kernels
 * conv_small_kernel / conv_wgrad_small_kernel with bn filters; bm = 1 -> conv_halo_kernel; bm = 2 -> conv_gather_pipe_kernel; bm = 4 ->
 * conv1x1_stream_kernel; bm = 5 -> conv1x1_regw_kernel, classes of bn = 192 filters resident in registers): lets a profiler-side caller
 * name the kernel a launch resolves to.  which = 2: the codes are computed from the weight-gradient choice (plan_wgrad, csrc/conv_wgrad.hip),
 * the one din_conv_wgrad launches from: bm = 3 -> conv_wgrad_halo_kernel with bn filter rows per class, bn = 2000 + k columns ->
 * conv_wgrad_pipe_kernel.  Several instantiations share a code (the tail kernel and conv_wgrad_bf16_kernel<128>; the stem forms):
 * din_conv_kernel_names(d, 2, ...) tells them apart */
int din_conv_kernel_tile(const din_conv_desc* d, int which, int32_t* bm, int32_t* bn);
/* which instantiation of conv_gather_fast_kernel a fwd (0) / dgrad (1) launch resolves to: flags bit 0 = FASTK (scalar k-walk), bit 1 = 8 waves
 * (4 x 2) instead of 4 (2 x 2) -- so that a profiler-side caller can spell the exact kernel name rocprofv3 prints */
int din_conv_kernel_variant(const din_conv_desc* d, int which, int32_t* flags);
/* the kernels din_conv_fwd (which 0) / din_conv_dgrad (which 1) launch for this descriptor, flags and mask view (ldm, moff: read for
 * DIN_CONV_MASK only), under the current option settings: one line per launch, in launch order, each the full template instantiation as the
 * launcher spells it -- "conv_gather_fast_kernel<bf16,128,192,4,2,8,2,0,1,0,0>" (T, BM, BN, WM, WN, KCS, NS, MULTI, FASTK, XSRC, LANEK),
 * "conv_gather_generic_kernel<float,128>", "conv_small_kernel<8,32,1,3,3,1,0,8,1>", "conv_halo_kernel<80,3,3,8,32,2,16>",
 * "conv_gather_pipe_kernel<192>", "conv1x1_stream_kernel<96,4,0,1,0>", "conv1x1_regw_kernel<24,1,9,1,3>", and "conv_splitk_finish_kernel<bf16>"
 * after a launch whose reduction is split.  A strided data gradient gives the line(s) of every non-empty parity class.  Host only: answers
 * from the launcher's own selection, launches nothing, reads no pointer, needs no GPU.  Writes at most buf_bytes bytes (NUL-terminated) and
 * returns the number of bytes the whole answer needs (terminator included), or a negative DIN_E_* code.  (din_conv_fwd2,
 * din_conv1x1_dgrad_multi and din_conv_dgrad_x have reporters of their own, declared after them: din_conv_fwd2_kernel_names, ...)
 * which 2: the launches of a production-style din_conv_wgrad call (dbias, scale, w and wdot given) under the current options, from the
 * weight-gradient choice din_conv_wgrad itself launches from: the main kernel, "conv_wgrad_reduce_kernel", and the column-sum kernel
 * ("colsum_vec_kernel<unsigned short, 8>", "colsum_kernel<float>", ...) where the main kernel does not sum the bias gradient itself.  flags,
 * ldm and moff must be 0 (DIN_E_ARG otherwise).  These lines are spelled DIFFERENTLY from the forward / data-gradient ones, on purpose: as the
 * demangler spells the instantiation, which is what rocprofv3 prints -- every template argument with the defaults written out, ", "
 * between them, true / false for bools ("conv_wgrad_small_kernel<4, 64, 1, false, 8, 6, 3>", "conv_wgrad_pipe_kernel<192, 256, true, 8>",
 * "conv_wgrad_halo_kernel<8, 48, 3, 3, 8>", "conv_wgrad_ring_kernel<64, 128>", "conv_wgrad_bf16_kernel<128>", "conv_wgrad_bf16_tail_kernel",
 * "conv_wgrad_f32_kernel") -- because profiling.LaunchTimer and the benchmark's dominant-kernel string use the first line verbatim. */
int din_conv_kernel_names(const din_conv_desc* d, int which, int flags, int ldm, int moff, char* buf, int buf_bytes);
/* workspace bytes needed by fwd / dgrad / wgrad for this descriptor (split-K partial sums) */
int64_t din_conv_workspace_bytes(const din_conv_desc* d, int which /*0 fwd,1 dgrad,2 wgrad*/);

/* 1 when both the forward and the weight-gradient launch of this layer run the image-layer kernels that can read uint8 frames directly
 * (bf16, 3x3 stride 2, <= 8 input channels, <= 32 filters, >= 256 Ki output pixels); 0 otherwise (prepare the input with
 * din_prep_images_nhwc).  Host-only planning call. */
int din_conv_accepts_u8(const din_conv_desc* d);

int din_conv_fwd(const din_conv_desc* d, const void* in, const void* wpk, const float* bias, void* out,
                 int flags, void* workspace, int64_t workspace_bytes, void* stream);
/* dout has the OUTPUT geometry of d (pixel stride ldo/cooff); din gets the INPUT geometry (ldi/cioff).   */
int din_conv_dgrad(const din_conv_desc* d, const void* dout, const void* wpk_t, void* din,
                   const void* mask, int ldm, int moff, int flags,
                   void* workspace, int64_t workspace_bytes, void* stream);
/* The filter-stationary halo kernel (csrc/conv_halo_rf.hip) for the narrow 3x3 layers: bf16, 3x3, stride 1, dilation 1, reduction and
 * produced channels in 40..96 at multiples of 8; forward (BIAS / RELU) and data gradient (MASK / ACCUM; the mask view at multiples of 8).
 * It is NOT reachable through din_conv_fwd / din_conv_dgrad: the caller asks din_conv_rf_eligible once per launch (host only, reads no
 * pointer: 1 = din_conv_rf_fwd / din_conv_rf_dgrad serve this launch and the planner wants it there, 0 = call din_conv_fwd / din_conv_dgrad)
 * and then calls the matching entry, which takes the argument list of din_conv_fwd / din_conv_dgrad (the workspace is not used) and
 * computes the same result.  A launch that is not eligible is DIN_E_ARG from the entries and the reporter, never another kernel.
 * Options: DIN_CONV_HALO_RF = 0 off, unset the planner's rule (a floor on the pixels of the launch, profiles/halo_rf_layers.txt), 2 every
 * eligible shape; DIN_CONV_HALO = 0 switches it off as well.  din_conv_rf_kernel_names answers like din_conv_kernel_names, with the kernel
 * spelled as rocprofv3 prints it ("conv_halo_rf_kernel<3, 3, true>": 16-row filter tiles per wave, 32-channel steps per tap, data gradient). */
int din_conv_rf_eligible(const din_conv_desc* d, int which /*0 fwd,1 dgrad*/, int flags, int ldm, int moff);
int din_conv_rf_fwd(const din_conv_desc* d, const void* in, const void* wpk, const float* bias, void* out,
                    int flags, void* workspace, int64_t workspace_bytes, void* stream);
int din_conv_rf_dgrad(const din_conv_desc* d, const void* dout, const void* wpk_t, void* din,
                      const void* mask, int ldm, int moff, int flags,
                      void* workspace, int64_t workspace_bytes, void* stream);
int din_conv_rf_kernel_names(const din_conv_desc* d, int which, int flags, int ldm, int moff, char* buf, int buf_bytes);
/* The same for the narrow 5x5 layers (csrc/conv_halo_rf5.hip): bf16, 5x5, stride 1, dilation 1, oh = h + 2 ph - 4, reduction and produced
 * channels in 40..64 at multiples of 8; forward (BIAS / RELU) and data gradient (MASK / ACCUM; the mask view at multiples of 8).  One
 * corner is not served: a MASKED data gradient with 56 or 64 reduction channels AND more than 48 produced channels (halo buffers and mask
 * regions would exceed the LDS).  A family of its own, not reached through din_conv_rf_*: the caller asks din_conv_rf5_eligible and calls
 * din_conv_rf5_fwd / din_conv_rf5_dgrad, which take the argument lists of their rf counterparts.  Options: DIN_CONV_HALO_RF5 = 0 off, unset
 * the planner's rule (a floor on the pixels of the launch, profiles/halo_rf5_layers.txt; no ACCUM), 2 every eligible shape; DIN_CONV_HALO = 0
 * switches it off as well.  Kernel names: "conv_halo_rf5_kernel<6, false>" (16-byte chunks per tap of the reduction, data gradient). */
int din_conv_rf5_eligible(const din_conv_desc* d, int which /*0 fwd,1 dgrad*/, int flags, int ldm, int moff);
int din_conv_rf5_fwd(const din_conv_desc* d, const void* in, const void* wpk, const float* bias, void* out,
                     int flags, void* workspace, int64_t workspace_bytes, void* stream);
int din_conv_rf5_dgrad(const din_conv_desc* d, const void* dout, const void* wpk_t, void* din,
                       const void* mask, int ldm, int moff, int flags,
                       void* workspace, int64_t workspace_bytes, void* stream);
int din_conv_rf5_kernel_names(const din_conv_desc* d, int which, int flags, int ldm, int moff, char* buf, int buf_bytes);
/* Fused dgrad of up to four 1x1 / stride-1 convolutions that read the SAME tensor (the branch-entry convs of torchvision's
 * InceptionA/C blocks, backbone.py:61-77): din = sum_b dout_b . W_b^T computed as ONE contraction over the concatenated
 * channels, so the (write-bound) gradient tensor is written once instead of once per branch with read-modify-write.
 * Source b: dout_b [nb,h,w,cout_b] (pixel stride ldo, offset cooff), wpk_t = its bank packed with transposed=1.       */
typedef struct din_conv_src {
    const void* dout;
    const void* wpk_t;
    int32_t cout, ldo, cooff;
} din_conv_src;
int din_conv1x1_dgrad_multi(int nsrc, const din_conv_src* srcs, int dtype, int nb, int h, int w, int cin, int ldi,
                            int cioff, void* din, const void* mask, int ldm, int moff, int flags, void* stream);
/* din_conv_dgrad of a STRIDED conv plus the dgrad of ONE 1x1 / stride-1 conv `x` that reads the same input view, in the same launches:
 * din (op)= mask(conv^T(dout) + conv1x1^T(x->dout)).  torchvision's InceptionB (backbone.py MyInception_v3 Mixed_6a, through torchvision
 * inception.py InceptionB.forward: branch3x3 = 3x3 stride 2 and branch3x3dbl_1 = 1x1 both read the block input): the 1x1's 64 channels ride
 * as one more k-step of the four parity-class launches of the 3x3, so the 288-channel gradient map is read-modify-written once, not twice.
 * x->wpk_t = the 1x1's bank packed with transposed=1 (as for din_conv1x1_dgrad_multi).  Shapes the fused kernel does not serve (fp32,
 * stride 1, tiles other than 128 x 96, split-K; DIN_DGRAD_X=0) run as din_conv_dgrad followed by din_conv1x1_dgrad_multi with ACCUM --
 * same result up to the rounding of the intermediate sum.                                                                      */
int din_conv_dgrad_x(const din_conv_desc* d, const void* dout, const void* wpk_t, void* din, const void* mask, int ldm, int moff, int flags,
                     const din_conv_src* x, void* workspace, int64_t workspace_bytes, void* stream);
/* 1 when din_conv_dgrad_x serves this descriptor with the fused kernel, 0 when it runs the two-launch form.  Host-only planning call. */
int din_conv_dgrad_x_fused(const din_conv_desc* d);
/* din_conv_kernel_names for the three multi-source / two-destination entry points: the kernels din_conv_fwd2, din_conv1x1_dgrad_multi and
 * din_conv_dgrad_x launch for these arguments under the current option settings, spelled and returned as din_conv_kernel_names does (one
 * line per launch, in launch order; at most buf_bytes bytes written, the bytes the whole answer needs returned, or a negative DIN_E_*
 * code).  Host only: each answers from the very function its entry point builds its argument block, plan and choice in, launches nothing,
 * needs no GPU and reads no pointer -- of a din_conv_src only cout, ldo and cooff.  The argument checks are the entry point's own (a
 * din_conv_fwd2 shape that would run split-K is DIN_E_ARG from both).  din_conv_dgrad_x_kernel_names gives the parity-class lines of the
 * fused form ("conv_gather_fast_kernel<bf16,128,96,4,2,8,2,0,0,1,0>" each) and, where din_conv_dgrad_x_fused() is 0, the lines of the
 * din_conv_dgrad launch followed by those of the one-source din_conv1x1_dgrad_multi launch (flags | DIN_CONV_ACCUM). */
int din_conv_fwd2_kernel_names(const din_conv_desc* d, int ldo2, int cooff2, int csplit, int craw, int flags, char* buf, int buf_bytes);
int din_conv1x1_dgrad_multi_kernel_names(int nsrc, const din_conv_src* srcs, int dtype, int nb, int h, int w, int cin, int ldi, int cioff,
                                         int ldm, int moff, int flags, char* buf, int buf_bytes);
int din_conv_dgrad_x_kernel_names(const din_conv_desc* d, const din_conv_src* x, int ldm, int moff, int flags, char* buf, int buf_bytes);
/* dw: [cout][cin][kh][kw] fp32, overwritten (or += when accumulate bit 0 (value 1) is set; bit 1 alone leaves dw overwritten),
 * multiplied by scale[cout] when scale is given.  dbias (nullable) [cout] fp32 = column sums of dout.  wdot (nullable) [cout] fp32 =
 * <w[co,:], dw_raw[co,:]> (needs w) -- the BatchNorm-eval scale gradient.  accumulate bit 1 (value 2): dbias / wdot were zeroed by
 * the caller (they are accumulated into with atomics; a backbone zeroes one flat buffer for all its layers instead of 2 memsets per
 * layer).                                                                                                   */
int din_conv_wgrad(const din_conv_desc* d, const void* in, const void* dout, float* dw, float* dbias,
                   const float* scale, const float* w, float* wdot, int accumulate,
                   void* workspace, int64_t workspace_bytes, void* stream);

/* Weight gradients of 2..4 1x1 / stride-1 convs that read the SAME tensor view (the block-entry convs of an InceptionA block, reference
 * backbone/backbone.py:44-58 through torchvision: branch1x1, branch5x5_1 + branch3x3dbl_1, branch_pool) in ONE launch: the input is read
 * once instead of once per layer, every layer's dW block stays in registers of persistent workgroups (csrc/conv_wgrad_1x1.hip).
 * Source b: dout_b [pixels][ldo] at channel cooff (its gradient operand), dw_b [cout_b][cin] fp32, and din_conv_wgrad's optional
 * dbias / scale / w / wdot of that layer.  din_conv1x1_wgrad_multi_workspace returns the workspace bytes, or 0 when the group does not
 * fit the kernel (bf16, cin in {192, 256, 288}, couts multiples of 16 that can be dealt to two classes of <= 128 rows, >= 128K pixels):
 * the caller then runs din_conv_wgrad per layer.  accumulate as in din_conv_wgrad.                                              */
typedef struct din_conv_wsrc {
    const void* dout;
    float* dw;
    float* dbias;
    const float* scale;
    const float* w;
    float* wdot;
    int32_t cout, ldo, cooff;
} din_conv_wsrc;
int64_t din_conv1x1_wgrad_multi_workspace(int nsrc, const din_conv_wsrc* srcs, int dtype, int64_t pixels, int cin);
int din_conv1x1_wgrad_multi(int nsrc, const din_conv_wsrc* srcs, int dtype, int64_t pixels, int cin, int ldi, int cioff, const void* in,
                            int accumulate, void* workspace, int64_t workspace_bytes, void* stream);
/* din_conv_kernel_names for din_conv1x1_wgrad_multi: "conv_wgrad_1x1_multi_kernel<CPP>" (CPP = cin / 8) and one "conv_wgrad_reduce_kernel"
 * line per source, in launch order, spelled and returned as din_conv_kernel_names(d, 2, ...) does.  Host only: answers from the function the
 * launch plans in and the table it launches from, reads of a din_conv_wsrc only cout, ldo and cooff.  A group the kernel does not take
 * (din_conv1x1_wgrad_multi_workspace answers 0) is DIN_E_ARG, as from the launch. */
int din_conv1x1_wgrad_multi_kernel_names(int nsrc, const din_conv_wsrc* srcs, int dtype, int64_t pixels, int cin, char* buf, int buf_bytes);

/* The weight gradients of up to 16 LAYERS in one launch (autograd of the torch.nn.Conv2d layers of reference backbone/backbone.py:44-99 --
 * torchvision's InceptionC blocks hold ten 7-tap / 1x1 layers of equal map size each).  A weight-gradient launch of the pipelined kernel puts
 * one workgroup on every CU and each writes a full fp32 partial tile: slices x |dW| = ~50 MB per layer whatever the batch, read back by the
 * reduce launch.  Layers whose gradients are due at about the same time share one launch and its 256 workgroups instead: a layer of a group
 * of six is cut into 7 instead of 42 pixel slices (8 MB of partials), and the launch has one tail instead of six.
 * An item = the arguments of one din_conv_wgrad call.  din_conv_wgrad_group_key: 0 = this layer's gradient does not run on the pipelined
 * kernel (it cannot join a group); items with EQUAL non-zero keys may share a launch.  din_conv_wgrad_group_workspace: bytes for this group,
 * 0 = not a valid group (the caller runs din_conv_wgrad per item; din_conv_wgrad_group itself does the same when handed such a list, with
 * a workspace that must then hold the largest single-item need).  Results equal din_conv_wgrad's up to the order of the slice sums. */
typedef struct din_conv_wgrad_item {
    din_conv_desc desc;
    const void* in;
    const void* dout;
    float* dw;
    float* dbias;
    const float* scale;
    const float* w;
    float* wdot;
    int32_t accumulate, reserved;
} din_conv_wgrad_item;
int din_conv_wgrad_group_key(const din_conv_desc* d);
int64_t din_conv_wgrad_group_workspace(int n, const din_conv_wgrad_item* items);
int din_conv_wgrad_group(int n, const din_conv_wgrad_item* items, void* workspace, int64_t workspace_bytes, void* stream);
/* din_conv_kernel_names for din_conv_wgrad_group, host only, from the group plan the launch itself makes (of an item only desc is read):
 * "conv_wgrad_pipe_group_kernel<BCO, 256, WIDE, 8>" and "conv_wgrad_reduce_group_kernel" for a list that runs as one launch; for a list
 * that runs layer by layer (n = 1, n > 16, unequal or zero keys) the lines of din_conv_kernel_names(&item.desc, 2) item after item.
 * din_conv_wgrad_group_slices: the plan's pixel slices per item (the first min(n, cap) written to slices[]); returns the slice groups of
 * the reduce launch's workgroups (1, 4 or 16: chosen from the largest slice count), 0 for a list that runs layer by layer, or a negative
 * DIN_E_* code. */
int din_conv_wgrad_group_kernel_names(int n, const din_conv_wgrad_item* items, char* buf, int buf_bytes);
int din_conv_wgrad_group_slices(int n, const din_conv_wgrad_item* items, int32_t* slices, int cap);

/* out[c] = sum over rows of g[row*ld + coff + c] (fp32 result; BatchNorm shift gradient of a conv whose epilogue ran in the pool) */
int din_colsum(const void* g, int dtype, int64_t rows, int c, int ld, int coff, float* out, void* stream);

/* BatchNorm(eval) folding helpers (torchvision BasicConv2d, eps=1e-3; train_net_dynamic.py:17-20 set_bn_eval)
 * scale = gamma*rsqrt(var+eps); shift = beta - mean*scale                                                */
int din_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                float* scale, float* shift, int c, void* stream);
/* dgamma = (wdot - dshift*mean)*rsqrt(var+eps); dbeta = dshift                                            */
int din_bn_fold_bwd(const float* wdot, const float* dshift, const float* mean, const float* var, float eps,
                    float* dgamma, float* dbeta, int c, void* stream);
/* The same two maps for ALL BatchNorm layers of a backbone in one launch each.  Device tables: ptrs [n][4] = addresses of
 * {gamma, beta, running_mean, running_var} per layer; offs [n+1] = prefix sums of the channel counts (offs[n] = total).  scale / shift /
 * wdot / dshift / dgamma / dbeta are flat [total] fp32 arrays, layer l owning [offs[l], offs[l+1]). */
int din_bn_fold_multi(const uint64_t* ptrs, const int32_t* offs, int n, int total, float eps, float* scale, float* shift,
                      void* stream);
int din_bn_fold_bwd_multi(const uint64_t* ptrs, const int32_t* offs, int n, int total, float eps, const float* wdot,
                          const float* dshift, float* dgamma, float* dbeta, void* stream);

/* BatchNorm with BATCH statistics: the reference's default for the Inception-v3 backbone in stage 2 -- model.train() without
 * set_bn_eval (train_net_dynamic.py:98-100,170-172; config.py:80) -> torch.nn.functional.batch_norm(training=True) inside torchvision's
 * BasicConv2d.  Views are [rows][c] with pixel stride ld and channel offset coff (elements; multiples of 4 fp32 / 8 bf16).
 * Workspace ws (fp64, din_bn_workspace(rows, c) bytes, NOT zeroed by the caller): ws[0..2c) = the reduced sums, then din_bn_parts(rows)
 * slabs of 2c partial sums, one per workgroup of the statistics kernel.  Everything is summed in a fixed order (fp64 per-thread
 * accumulators with exact products, lane-ordered LDS sum, slab-ordered reduce): the same input gives the same bits on every run.
 *   din_bn_stats     : slab[p][0..c) = sum over the rows of part p of (x - shift), slab[p][c..2c) = sum (x - shift)^2   (shift [c] nullable
 *                      = 0; fp64 accumulation makes it unnecessary -- kept for callers that have one; din_bn_finalize must get the SAME)
 *   din_bn_finalize  : ws[0..2c) = slab sums in slab order (nparts > 0; nparts == 0: ws[0..2c) already holds them); mean,
 *                      rstd = 1/sqrt(biased var + eps); a = gamma*rstd, b = beta - mean*a; running_mean/var (may be NULL) updated
 *                      in place with `momentum` and the unbiased variance, as torch does
 *   din_bn_apply     : y = a*x + b (relu != 0: max(.,0)) -- x and y may be views of different tensors
 *   din_bn_bwd_stats : ws[0..c) = sum gz, ws[c..2c) = sum gz*xhat, xhat = (x - mean)*rstd   (gz: gradient at the BN output,
 *                      already masked by the ReLU that follows); slabs + din_bn_reduce inside
 *   din_bn_reduce    : ws[0..2c) = sum of nparts slabs at ws + 2c, in slab order (for producers that fill the slabs themselves)
 *   din_bn_bwd_apply : dy = gamma*rstd*(gz - s1/rows - xhat*s2/rows); dgamma = s2, dbeta = s1   (sums = ws of din_bn_bwd_stats)        */
int din_bn_parts(int64_t rows);
int64_t din_bn_workspace(int64_t rows, int c);
int din_bn_stats(const void* x, int dtype, int64_t rows, int c, int ld, int coff, const float* shift, double* ws, void* stream);
int din_bn_reduce(double* ws, int nparts, int c, void* stream);
int din_bn_finalize(double* ws, int nparts, int64_t rows, int c, const float* gamma, const float* beta, float eps, float momentum,
                    float* running_mean, float* running_var, float* a, float* b, float* mean, float* rstd, const float* shift,
                    void* stream);
int din_bn_apply(const void* x, int dtype, int64_t rows, int c, int ldx, int cxoff, const float* a, const float* b, int relu,
                 void* y, int ldy, int cyoff, void* stream);
int din_bn_bwd_stats(const void* gz, int ldg, int cgoff, const void* x, int ldx, int cxoff, int dtype, int64_t rows, int c,
                     const float* mean, const float* rstd, double* ws, void* stream);
int din_bn_bwd_apply(const void* gz, int ldg, int cgoff, const void* x, int ldx, int cxoff, int dtype, int64_t rows, int c,
                     const float* gamma, const float* mean, const float* rstd, const double* sums, void* dy, int ldy, int cyoff,
                     float* dgamma, float* dbeta, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pools / resize (backbone.py:51,57 max_pool2d; torchvision InceptionA/C avg_pool2d(3,1,1), InceptionB
 * max_pool2d(3,2); vgg.features MaxPool2d(2,2); infer_model.py:169 F.interpolate bilinear align_corners)
 * ---------------------------------------------------------------------------------------------- */
typedef struct din_pool_desc {
    int32_t nb, h, w, c, oh, ow;
    int32_t k, stride, pad;
    int32_t ldi, cioff, ldo, cooff;
    int32_t dtype;
} din_pool_desc;
/* argmax (nullable): uint8 [nb,oh,ow,c] map of the winning tap r*k+s (first maximum, PyTorch's tie rule), 255 when the
 * winner is <= 0 -- i.e. the map already carries the fused ReLU-backward mask of the tensor being pooled.            */
int din_maxpool_fwd(const din_pool_desc* d, const void* in, void* out, uint8_t* argmax, void* stream);
/* din = scatter of dout to the first maximal element of each window; relu_mask!=0 additionally multiplies by
 * (in > 0) -- the fused backward of the ReLU that produced `in`.  accumulate!=0: din += ...
 * With argmax (saved by the forward; requires relu_mask!=0) `in` is not read at all; without it the window arg-max
 * is recomputed from `in`.                                                                                          */
int din_maxpool_bwd(const din_pool_desc* d, const void* in, const uint8_t* argmax, const void* dout, void* din_,
                    int relu_mask, int accumulate, void* stream);
/* F.avg_pool2d(x, k, stride, pad) with count_include_pad (backbone: torchvision InceptionA/C branch_pool).  flags: DIN_CONV_BIAS adds
 * bias[c] (fp32) after the average, DIN_CONV_RELU clamps: the epilogue of a 1x1 conv commuted in front of the pool
 * (avgpool(conv1x1(x)) == conv1x1(avgpool(x)), both linear, zero padding maps to zero) -- the pool then runs on cout channels */
int din_avgpool_fwd(const din_pool_desc* d, const void* in, void* out, const float* bias, int flags, void* stream);
int din_avgpool_bwd(const din_pool_desc* d, const void* dout, void* din_, const void* mask, int accumulate,
                    void* stream);
int din_bilinear_fwd(const din_pool_desc* d, const void* in, void* out, void* stream); /* align_corners=True */
int din_bilinear_bwd(const din_pool_desc* d, const void* dout, void* din_, const void* mask, int accumulate,
                     void* stream);
/* host-only: writes the name of the kernel instantiation the launch resolves to, exactly as it is spelled at the launch site
 * ("maxpool3s2_row_bwd_kernel<256, true>"), from the decision function the launchers themselves switch on -- for tests and for a
 * profiler-side caller that wants to spell the name rocprofv3 prints.  has_argmax / accumulate matter to din_maxpool_bwd only. */
int din_pool_kernel_name(const din_pool_desc* d, int op /*0 maxpool,1 avgpool,2 bilinear*/, int backward, int has_argmax,
                         int accumulate, char* buf, int buf_bytes);

/* ------------------------------------------------------------------------------------------------
 * Row R  RoIAlign(K,K) = TF crop_and_resize, transform_fpcoor=True (third-party longcw/RoIAlign.pytorch;
 * call site infer_model.py:178-180), optionally composed with the multi-scale fuse in front of it
 * (infer_model.py:165-172: F.interpolate(size=(OH,OW), mode='bilinear', align_corners=True) + torch.cat).
 * fm: the STORED map, NHWC [nb,hf,wf,c] (dtype fm_dtype, pixel stride ldf).  (gh,gw): the grid the boxes are expressed on.
 * gh==hf && gw==wf is the plain RoIAlign; a larger grid means "fm virtually resized to gh x gw with align_corners": each sample
 * is then a 3x3 weighted sum of stored pixels (both operations are separable and linear) and the resized map is never materialised.
 * boxes [m,4]=(x1,y1,x2,y2) grid px fp32; box_ind [m] int32; out fp32 [m][out_c][k][k] (the reference's flatten order
 * d,ky,kx: infer_model.py:181), this map's c channels at [out_coff, out_coff+c) -- one call per source of the torch.cat.
 * idx_out (nullable, plain sampling only) int32 [m][k][6] = (top,bottom,left,right,oob_y,oob_x) per sample row/col for
 * bit-exact index tests.
 * ---------------------------------------------------------------------------------------------- */
int din_roi_align_fwd(const void* fm, int fm_dtype, int nb, int hf, int wf, int c, int ldf, int gh, int gw,
                      const float* boxes, const int32_t* box_ind, int m, int k,
                      float* out, int out_c, int out_coff, int32_t* idx_out, void* stream);
/* dfm fp32 [nb,hf,wf,c] must be zeroed by the caller; 4-corner atomic scatter; no gradient to boxes */
int din_roi_align_bwd(const float* dout, int nb, int hf, int wf, int c,
                      const float* boxes, const int32_t* box_ind, int m, int k,
                      float* dfm, void* stream);
/* crop gradient [m][c][k*k] (the reference's flatten order = the column order of fc_emb_1) -> channel-contiguous [m][k*k][c]: the
 * gather backward then reads 16/32-byte runs instead of 4-byte loads 4*k*k bytes apart.  One call serves every source map. */
int din_roi_crop_grad_transpose(const float* dout, int m, int c, int k, float* out, void* stream);
/* Gather form of the gradient, written once into the stored map's gradient view gfm [nb,hf,wf,ldg] (storage `dtype`, channels
 * [0,c), every pixel -- zeros outside the boxes): no atomics, no fp32 staging tensor, no zero-fill, deterministic summation order.
 * dout: the crop gradient with dout_c channels per crop, this map's at [dout_coff, dout_coff+c); layout [m][dout_c][k*k], or
 * [m][k*k][dout_c] when `transposed` (din_roi_crop_grad_transpose).  (gh,gw) as in din_roi_align_fwd: with a larger grid this is the
 * fused backward of RoIAlign AND the bilinear resize.
 * fm_mask (nullable, same dtype, pixel stride ldf): the stored map; gradients are multiplied by (fm_mask > 0) -- the fused
 * backward of the ReLU that produced it.  box_ind may be in any order. */
int din_roi_align_bwd_nhwc(const float* dout, int dout_c, int dout_coff, int transposed, int nb, int hf, int wf, int c,
                           int gh, int gw, const float* boxes, const int32_t* box_ind, int m, int k,
                           const void* fm_mask, int dtype, int ldf, void* gfm, int ldg, void* stream);
/* fp32 gradient map -> backbone dtype, fused with the ReLU mask of the feature map that was cropped */
int din_grad_cast_mask(const float* g, const void* y, void* out, int dtype, int64_t pixels, int c,
                       int ldy, int yoff, int ldo, int ooff, int use_mask, void* stream);
/* builds box_ind[i*n+j] = i (infer_model.py:155-157) */
int din_boxes_frame_index(int32_t* out, int bt, int n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SURVEY 8(f)-4  Context-encoding transformer of Dynamic_TCE_volleyball (infer_model.py:404-410;
 * infer_module/TCE_STBiP_module.py:252-286 EmbfeatureContextEncodingTransformer, :300-313 the 4-head layer).  fp32.
 * q [bt][n][heads*c] (emb_roi of every head), kf [bt][p][heads*c] (downsample2 of every head over the p = OH*OW context pixels),
 * s / a [bt][heads][n][p].  n <= 16 (the reference asserts 12), c a power of two <= 256 (128 in the reference).
 * ---------------------------------------------------------------------------------------------- */
/* s = <q, kf> per (frame, head, box, pixel): torch.matmul(emb_roi_feature, image_feature) (:271).  Also the backward's dA = <dctx, kf>. */
int din_ctx_scores(const float* q, const float* kf, float* s, int bt, int n, int p, int heads, int c, void* stream);
/* F.softmax(a, dim=2) (:273) in place over rows of `len`; backward in place on da: ds = a * (da - sum(a * da)) */
int din_softmax_rows(float* s, int64_t rows, int len, void* stream);
int din_softmax_rows_bwd(const float* a, float* da, int64_t rows, int len, void* stream);
/* out[bt][n][heads*c] = sum_p a * kf: torch.matmul(A, image_feature) (:277).  Also the backward's dq = sum_p ds * kf. */
int din_ctx_apply(const float* a, const float* kf, float* out, int bt, int n, int p, int heads, int c, void* stream);
/* dkf = a^T dctx + ds^T q: the gradient of both uses of the keys, written once */
int din_ctx_keys_grad(const float* a, const float* ds, const float* dctx, const float* q, float* dkf, int bt, int n, int p, int heads,
                      int c, void* stream);
/* Context_PositionEmbeddingSine.forward's last line (positional_encoding.py:91): y[f][i] = float(x[f][i]) + pos[i]; x in the backbone's
 * storage type (`dtype`), `per_frame` = OH*OW*C elements.  Backward: gx = cast(gy) (* (x > 0) when use_mask: the backbone graph takes
 * gradients that are already multiplied by the ReLU mask of its output) */
int din_add_position(const void* x, int dtype, const float* pos, float* y, int64_t frames, int64_t per_frame, void* stream);
int din_add_position_bwd(const float* gy, const void* x, int dtype, void* gx, int64_t elems, int use_mask, void* stream);
/* y = dropout(relu?(x)) (nn.ReLU + nn.Dropout of the FFN, TCE_STBiP_module.py:243-247; nn.Dropout on the attended context :277) with the
 * counter-based keep mask of din_layernorm_* (same seed + element index -> same mask in the backward) */
int din_act_dropout_fwd(const float* x, float* y, int64_t n, int relu, float drop_p, uint64_t seed, const uint64_t* seed_offset, void* stream);
int din_act_dropout_bwd(const float* gy, const float* x, float* gx, int64_t n, int relu, float drop_p, uint64_t seed,
                        const uint64_t* seed_offset, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm (+residual, +ReLU, +dropout): nl_emb_1 (infer_model.py:185), point_ln (:192), dpi_nl (:214),
 * hier_LN (dynamic_infer_module.py:493).  x, res: [rows][len]; gamma/beta [len]; eps 1e-5.
 * y = dropout(relu?(LN(x + res?)*gamma + beta)).  stats: [rows][2] = (mean, rstd) saved for backward.
 * dropout: keep-mask from a counter-based hash of (seed, element index), scale 1/(1-p); p=0 disables.
 * seed_offset (nullable, device memory): the mask seed is (seed + *seed_offset) mod 2^63, read by the kernel -- a training step captured
 * in a HIP graph bakes `seed` into the launch, so the part that changes per step lives in device memory (din_counter_add advances it
 * inside the graph); forward and backward of one step see the same value.
 * ---------------------------------------------------------------------------------------------- */
int din_layernorm_fwd(const float* x, const float* res, const float* gamma, const float* beta, float eps,
                      float* y, float* stats, int64_t rows, int64_t len, int relu, float drop_p,
                      uint64_t seed, const uint64_t* seed_offset, void* stream);
/* dx [rows][len] (also the gradient of res); dgamma/dbeta [len] are ACCUMULATED atomically (caller zeroes) */
int din_layernorm_bwd(const float* dy, const float* x, const float* res, const float* gamma,
                      const float* y, const float* stats, float* dx, float* dgamma, float* dbeta,
                      int64_t rows, int64_t len, int relu, float drop_p, uint64_t seed, const uint64_t* seed_offset, void* stream);
/* *counter += delta (one thread; stream-ordered): the per-step part of the dropout seeds of a graph-captured training step */
int din_counter_add(uint64_t* counter, uint64_t delta, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Rows D2-D4  Dynamic Relation + Dynamic Walk (dynamic_infer_module.py:184-282, 344-404), one module,
 * one sampling ratio.  x fp32 [b,t,n,c].  pred fp32 [b,t,n,cp] is the output of the fused
 * p_conv/scale_conv contraction (din_conv_fwd with cout = 3*k2: channels [0,k2) y-offsets, [k2,2k2)
 * x-offsets, [2k2,3k2) relation logits; cp = its pixel stride).  scale_factor=0 -> mean over k2, no logits.
 *   z   [b,t,n,c]      = sum_k a_k * S_k                   (:278 / :280)
 *   a   [b,t,n,k2]     = softmax_k(logits)  (saved)        (:196)
 *   idx [b,t,n,k2,4]   int32 (ly,ry,lx,rx) clamped corners (:208-223)  -- bit-exact row
 *   mad (nullable) [b,t,n,k2,c] = S (ft_infer_MAD, :259); not materialised when NULL.
 * ---------------------------------------------------------------------------------------------- */
/*   n_per_clip (nullable) int32 [b]: clip i is a T x n_per_clip[i] grid held in the first columns of its T x n slab (Dynamic_collective,
 *   infer_model.py:1286-1293 runs the module per clip on boxes_features_all[b, :, :N]); columns beyond it are zero padding: they are
 *   read as zeros, get z = 0 and no gradient, and the x clamp range is the clip's own padded width.  x must already be zero there.
 *   The forward needs ONE padded (t+2pt) x (n+2pl) x 64-channel fp32 tile in LDS (<= 160 KiB, else DIN_E_ARG); the backward keeps a
 *   second one for the feature gradient when it fits and scatters into dx with global atomics when it does not.                 */
/*   plain != 0: no walk -- S_k is the feature at lattice point k itself (plain_infer_ratio :154-181 and the relation half of
 *   parallel_infer :285-298); the offset channels of pred are ignored and receive no gradient.  kh and kw must be odd (else
 *   DIN_E_ARG): with an even extent the reference's lattice leaves its own padded map.
 *   clamp (nullable HOST array of 4 ints {iy_max, ix_max, py_max, px_max}): clamp maxima of the corner indices and of the sampling
 *   position, for parallel_infer's walk half, which clamps with person_mat_shape (T + 2 ratio - 1, N + 2 ratio - 1; T + 2 ratio,
 *   N + 2 ratio: :307-317) instead of the padded grid; index maxima are additionally held inside the padded grid.              */
int din_walk_fwd(const float* x, const float* pred, int cp, int b, int t, int n, int c,
                 int kh, int kw, int ratio, int scale_factor, int plain, const int32_t* clamp, const int32_t* n_per_clip,
                 float* z, float* a, int32_t* idx, float* mad, void* stream);
/* gz [b,t,n,c] -> dx_walk [b,t,n,c] (overwritten), dpred [b,t,n,cp] (first 3*k2 channels written):
 * d offset through the |.| coefficients with detached floor (Q4), inclusive clamp pass-through (Q9),
 * sign(0)=0 (Q8); d logits through the softmax.  scratch: fp32 [ceil(c/64)][b,t,n,3*k2] (per-channel-chunk partial sums, written by the call).     */
int din_walk_bwd(const float* x, const float* pred, int cp, const float* a, const float* gz,
                 int b, int t, int n, int c, int kh, int kw, int ratio, int scale_factor, int plain, const int32_t* clamp,
                 const int32_t* n_per_clip, float* dx, float* dpred, float* scratch, void* stream);
/* host-only, launches nothing: the name of the kernel that forms the FEATURE gradient dx of a din_walk_bwd call of this shape under the
 * current options, from the decision code the launcher itself switches on: "din_walk_bwd_kernel<true>" (scatter into dx with fp32
 * atomics, the shipped choice), "din_walk_bwd_kernel<false>" (LDS tile, DIN_WALK_BWD_GLOBAL = 0 where two tiles fit) or, under
 * DIN_DETERMINISTIC, "din_walk_bwd_dx_ordered_kernel" (gather form: the terms of a destination cell -- the transposed torch.gather of
 * dynamic_infer_module.py:229-258 -- summed in (position, tap, corner) order, no atomics).  DIN_E_ARG where the launch would refuse.
 *
 * DIN_DETERMINISTIC = "1" (din_set_option; unset by default, and then nothing changes): din_walk_bwd, din_layernorm_bwd (dgamma /
 * dbeta), din_head_bwd (dw / dbias), din_dot_accum, din_colsum and the dbias of din_conv_wgrad produce results that are a pure function
 * of their arguments: no floating-point atomic, no sum whose order depends on scheduling, grid heuristics or other options.  A call that
 * has no such form under the option returns DIN_E_ARG naming it (a walk grid whose ordered kernel does not fit 160 KB of LDS;
 * din_conv_wgrad with wdot): never a silent fall-back.  The reference has no counterpart (it relies on cuDNN / ATen's defaults). */
int din_walk_bwd_kernel_name(int b, int t, int n, int c, int kh, int kw, int ratio, char* buf, int buf_bytes);

/* ------------------------------------------------------------------------------------------------
 * Row H  head (infer_model.py:224-232): max over actors -> fc_activities -> mean over frames.
 * s fp32 [b,t,n,c]; w [a,c]; bias [a]; argmax int32 [b,t,c] saved for backward.
 * scores: caller allocates b*a + b*t*a floats: [0, b*a) = clip scores [b,a], the tail = per-frame scores [b,t,a].
 * n_per_clip (nullable, int32 [b]) = number of valid actors of each clip (Collective: variable N).
 * ---------------------------------------------------------------------------------------------- */
int din_head_fwd(const float* s, const float* w, const float* bias, const int32_t* n_per_clip,
                 int b, int t, int n, int c, int a, float* scores, int32_t* argmax, void* stream);
/* ds overwritten; dw, dbias ACCUMULATED atomically (caller zeroes) */
int din_head_bwd(const float* dscores, const float* s, const float* w, const int32_t* argmax,
                 int b, int t, int n, int c, int a, float* ds, float* dw, float* dbias, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stage-1 base-model head (reference base_model.py:117-139 Basenet_volleyball, :243-268 Basenet_collective):
 *   s = dropout(relu(y)),  actions = s W_act^T + b_act (one row per valid box),  activities = max_boxes(s) W_grp^T + b_grp (per frame)
 * y fp32 [bt][n][c] (the fc_emb output; c <= 4096, n <= 256); w_act [a_act][c], w_grp [a_grp][c] (a_act, a_grp <= 16).  s is never
 * materialised: ReLU and the keep mask of din_act_dropout_fwd (same seed, same flat element index of y, optional seed_offset) are applied
 * on the fly, so s is bitwise din_act_dropout_fwd(y, relu=1).
 * mean_over_t != 0 (volleyball with T != 1, :135-137): t frames per clip, actions [bt/t*n][a_act] and activities [bt/t][a_grp] are the
 *   means over the clip's frames.  Otherwise actions [all_n][a_act], activities [bt][a_grp].
 * n_per_frame (nullable, device int32 [bt]): frame k holds n_per_frame[k] valid boxes (stage-1 collective counts per frame,
 *   train_net.py:284-290); action rows are compacted in (frame, box) order, offsets formed on the device.  all_n = number of action rows:
 *   bt/t*n (mean), bt*n (no n_per_frame) or the sum of n_per_frame, which the caller reads once from the device to size `actions`; a
 *   caller that finds a count outside 1..n passes all_n < 1 and gets DIN_E_ARG.
 * argmax int32 [bt][c]: the box of each channel's maximum (first maximum wins), saved for the backward.
 * Forward: ONE kernel launch.  Backward: ONE kernel launch, deterministic (fixed-order sums, no atomics): g_y [bt][n][c] overwritten
 *   (zero for padding boxes), dw_act / db_act / dw_grp / db_grp overwritten.  g_actions / g_activities have the forward's output shapes.
 * ---------------------------------------------------------------------------------------------- */
int din_basenet_head_fwd(const float* y, const float* w_act, const float* b_act, const float* w_grp, const float* b_grp,
                         const int32_t* n_per_frame, int all_n, int bt, int t, int mean_over_t, int n, int c, int a_act, int a_grp,
                         float drop_p, uint64_t seed, const uint64_t* seed_offset, float* actions, float* activities, int32_t* argmax,
                         void* stream);
int din_basenet_head_bwd(const float* g_actions, const float* g_activities, const float* y, const float* w_act, const float* w_grp,
                         const int32_t* argmax, const int32_t* n_per_frame, int all_n, int bt, int t, int mean_over_t, int n, int c,
                         int a_act, int a_grp, float drop_p, uint64_t seed, const uint64_t* seed_offset, float* g_y, float* dw_act,
                         float* db_act, float* dw_grp, float* db_grp, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Actor Relation Graph block (reference infer_module/ARG_infer_module.py:46-89 GCN_Module), everything after the projections.
 *   theta, phi fp32 [b][tn][ng][nfr] and y fp32 [b][tn][ng][nfg] with ROW STRIDE ld floats between consecutive (b, tn) rows: column slices
 *   of one projection output X [W_theta | W_phi | W_gcn]^T (y_g = X W_gcn,g^T; the graph is applied after it: R (X W^T) == (R X) W^T).
 *   boxes fp32 [b][tn][4] (x1, y1, x2, y2) in feature px; centre_rounds = how often the reference's in-place update
 *   col0 = (col0 + col2) / 2, col1 = (col1 + col3) / 2 (:48-49, once per GCN layer on the caller's tensor) has run when this layer reads
 *   the centres: layer l passes l + 1; the caller's boxes are not written.  thr = pos_threshold * OW (>= 0).
 *   gamma, beta fp32 [ng][tn][nfg] (nl_gcn_list), eps of the LayerNorm.
 * Per (clip, graph): S = theta phi^T / sqrt(nfr); S[i][j] = -inf where i != j and dist(centre_i, centre_j) > thr (strict; a NaN distance
 *   is kept); R = softmax over j; Z = R y_g; V = relu(LayerNorm over the whole [tn][nfg] slab (Z) * gamma_g + beta_g).
 * Outputs: out [b][tn][nfg] = sum of V over the graphs in order; rel [b][ng][tn][tn] = R of every graph (rel[:, ng-1] is the module's
 *   second return value); mask uint8 [b][tn][tn] (1 = masked); z [b][ng][tn][nfg] and stats [b][ng][2] = (mean, rstd), kept for the backward.
 * ws: ws_floats >= b * ng * ceil(nfg / 64) * 3 floats of scratch.
 * Limits: 1 <= tn <= 120; 1 <= ng <= 1024; nfr, nfg, ld multiples of 4; theta / phi / y 16-byte aligned; b * ng <= 65535; else DIN_E_ARG, nothing is read.
 * Forward 4 launches, backward 5; deterministic (fixed-order sums, no atomics), fp32 throughout.
 * Backward: g_out [b][tn][nfg] -> d_theta, d_phi, d_y (same column layout, row stride ld_grad, every element of the three slices written),
 *   d_gamma, d_beta [ng][tn][nfg] overwritten.  ws: ws_floats >= b*ng*tn*nfg + roundup4(b*ng*ceil(nfg/64)*2) + b*ng*tn*tn, 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
int din_arg_graph_fwd(const float* theta, const float* phi, const float* y, int64_t ld, const float* boxes, int centre_rounds, float thr,
                      const float* gamma, const float* beta, float eps, int b, int tn, int ng, int nfr, int nfg, float* out, float* rel,
                      uint8_t* mask, float* z, float* stats, float* ws, int64_t ws_floats, void* stream);
int din_arg_graph_bwd(const float* g_out, const float* theta, const float* phi, const float* y, int64_t ld, const float* gamma,
                      const float* beta, const float* rel, const float* z, const float* stats, int b, int tn, int ng, int nfr, int nfg,
                      float* d_theta, float* d_phi, float* d_y, int64_t ld_grad, float* d_gamma, float* d_beta, float* ws, int64_t ws_floats,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * Actor-Transformer block (the AT baseline): box-centre position embedding and single-head actor self-attention.
 *
 * Position (reference infer_module/AT_infer_module.py:52-96 Embfeature_PositionEmbedding): x fp32 [b][t][n][c], boxes fp32 [b][t][n][4]
 *   (x1, y1, x2, y2) in feature px, dim_t fp32 [c/2] = temperature ** (2 * (i // 2) / (c/2)), built by the caller in fp32 exactly as the
 *   reference builds it (:82-83).  Centre (x1 + x2) / 2 * img_w / out_w, (y1 + y2) / 2 * img_h / out_h (:77-80); column k of the first half
 *   holds sin (k even) or cos (k odd) of centre_x / dim_t[k], the second half the same of centre_y (:85-90); true fp32 division and
 *   full-precision sinf / cosf (the arguments reach 1280 rad).  y = PE + x [b][t][n][c]; with pool_t != 0 y [b][n][c] is the mean of that
 *   over t (frames added in order, then divided by t): torch.mean(x, dim=1) of AT_infer_module.py:125-126 in the same pass.
 *   Backward: gx [b][t][n][c] = gy, or gy [b][n][c] / t when pool_t; the boxes get no gradient.
 *   Limits: b, t, n >= 1; c a positive multiple of 4; else DIN_E_ARG, nothing is read.  One launch each.
 *
 * Attention (AT_infer_module.py:130-138 Actor_Transformer.forward after the Q_W / K_W / V_W Linear layers, up to layernorm1): g groups of
 *   n <= 16 actors (the b*t frames, or the b clips after the t-mean).  q, k, v fp32 [g*n][c] with ROW STRIDE ld floats: three column blocks
 *   of ONE projection output X [Q_W | K_W | V_W]^T, as theta / phi / y of din_arg_graph_fwd; x fp32 [g][n][c] the block's input (residual).
 *   A = softmax over j of (q k^T / sqrt(c)), the row maximum subtracted;  Z = x + dropout(A v);  out = LayerNorm over c (Z) * gamma + beta.
 *   dropout: the counter-based keep mask of din_layernorm_* / din_act_dropout_* on the flat element index of out, scale 1/(1-p), drop_p = 0
 *   disables; seed_offset (nullable, device) as there.  keep (nullable) uint8 [g][n][c]: the keep mask, for inspection.
 *   Outputs: out [g][n][c]; att [g][n][n] = A; stats [g*n][2] = (mean, rstd); att and stats are all the backward keeps (Z and the mask are
 *   recomputed).
 *   Backward: g_out [g][n][c] -> d_q, d_k, d_v (row stride ld_grad, every element of the three blocks written: the projection's data and
 *   weight gradients stay one contraction each), d_x [g][n][c] = gradient of the residual input, d_gamma / d_beta [c] overwritten:
 *   per-group partials in ws, then one reduce launch that adds the groups in order.  ws: ws_floats >= g * 2 * c.
 *   Limits: 1 <= n <= 16; c, ld, ld_grad multiples of 4, ld >= c; 0 <= drop_p < 1; q / k / v / x / out, g_out and the gradients 16-byte
 *   aligned, every other float pointer 4-byte aligned (seed_offset 8); no null pointer (keep and seed_offset excepted); else DIN_E_ARG, nothing is read or written.
 *   Forward 1 launch (one workgroup per group), backward 2; deterministic (fixed-order sums, no atomics), fp32 throughout.
 * ---------------------------------------------------------------------------------------------- */
int din_actor_position_fwd(const float* x, const float* boxes, const float* dim_t, float img_w, float img_h, float out_w, float out_h,
                           int b, int t, int n, int c, int pool_t, float* y, void* stream);
int din_actor_position_bwd(const float* gy, int b, int t, int n, int c, int pool_t, float* gx, void* stream);
int din_actor_attn_fwd(const float* q, const float* k, const float* v, int64_t ld, const float* x, const float* gamma, const float* beta,
                       float eps, float drop_p, uint64_t seed, const uint64_t* seed_offset, int g, int n, int c, float* out, float* att,
                       float* stats, uint8_t* keep, void* stream);
int din_actor_attn_bwd(const float* g_out, const float* q, const float* k, const float* v, int64_t ld, const float* x, const float* gamma,
                       const float* att, const float* stats, float drop_p, uint64_t seed, const uint64_t* seed_offset, int g, int n, int c,
                       float* d_q, float* d_k, float* d_v, int64_t ld_grad, float* d_x, float* d_gamma, float* d_beta, float* ws,
                       int64_t ws_floats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PCTDM baseline: the one-layer LSTM recurrence and the pooling / attention between its two LSTMs.
 *
 * LSTM (reference infer_module/pctdm_infer_module.py:23-24 Bi_Lstm and :47 Intra_Group_LSTM, run at :83 and :114), everything after the
 *   input projection.  pre fp32 [rows][steps][dirs][4*hidden] = x W_ih^T + b_ih + b_hh of all steps (one contraction by the caller), gate
 *   order i, f, g, o; w_hh fp32 [dirs][4*hidden][hidden]; dirs 1 or 2, direction 1 walks the positions steps-1 .. 0.  Zero initial state.
 *     z = pre + h W_hh^T;  i, f, o = sigmoid;  g = tanh;  c = f * c + i * g;  h = o * tanh(c)     (accurate expf / tanhf, true division)
 *   Outputs: h_out [rows][steps][dirs*hidden], torch's layout (position-major, forward half then reverse half, both at the position they
 *   belong to); gates [rows][steps][dirs][4*hidden] (activated) and cells [rows][steps][dirs][hidden], kept for the backward.
 *   One plain launch per step on the caller's stream, grid = (slices of 8 hidden units) x dirs: the step boundary is the all-to-all
 *   dependency; no grid-wide barrier, no cooperative launch, no workgroup waits for another.  A workgroup streams its 4 x 8 rows of w_hh with
 *   16-byte loads (4-byte loads when hidden % 4 != 0) against the previous h of 16 rows held in LDS; more rows are further chunks.
 *   Backward: g_out [rows][steps][dirs*hidden] -> d_pre [rows][steps][dirs][4*hidden] and h_prev [rows][steps][dirs][hidden] = the hidden
 *   state that entered each step (zeros at a direction's first step).  dW_hh is NOT formed here: it is one din_conv_wgrad per direction over
 *   the rows*steps rows with x = h_prev and gy = d_pre.  steps + 1 launches: w_hh^T into the workspace, then one launch per step in reverse
 *   walk order.  ws: ws_floats >= din_lstm_bwd_workspace(rows, dirs, hidden) = dirs*4*hidden^2 + rows*dirs*hidden floats.
 *   Limits: rows, steps >= 1; 1 <= hidden <= 1024; every pointer 16-byte aligned; else DIN_E_ARG, nothing is read or written.
 *   Deterministic (fixed-order sums, no atomics), fp32 throughout.
 *
 * Pool (pctdm_infer_module.py:94-96, :106): lstm_out fp32 [g][n][2*h] -> pooled [g][n][h] = max of the two direction halves of each player
 *   (the reference's view(g, 1, 2n, h) + MaxPool2d((2, 1)) pairs exactly those two rows; the first of two equal values wins),
 *   winner uint8 [g][n][h] (1 = the reverse half), context [g][h] = mean of pooled over n (players added in order, then divided by n).
 *   Backward: g_pooled [g][n][h], g_context [g][h] -> d_lstm_out [g][n][2*h], every element written.  One launch each; n <= 32.
 *
 * Attention (pctdm_infer_module.py:52-59 get_att_weigths, :112-114): pooled, src = att_source_weights(pooled) fp32 [g][n][h],
 *   ctx = att_context_weights(context) fp32 [g][h], w_e fp32 [h], b_e fp32 [1] (att_extra_weights, on the device).
 *     score[g][i] = <w_e, tanh(src[g][i] + ctx[g])> + b_e;  gamma = softmax of the scores inside each of the two teams of n / 2 players, the
 *     team's maximum subtracted;  y = pooled + pooled * gamma.
 *   Outputs: y [g][n][h], gamma [g][n].  Backward: g_y -> d_pooled, d_src [g][n][h], d_ctx [g][h], d_w_e [h], d_b_e [1], all overwritten;
 *   d_w_e / d_b_e are per-frame partials in ws, then one reduce launch that adds the frames in order (d_b_e is the plain sum of the score
 *   gradients: zero up to rounding, since a softmax ignores a common shift).  ws: ws_floats >= din_pctdm_att_bwd_workspace(g, h) = g*h + g.
 *   Limits: n even, 2 <= n <= 32; every pointer 4-byte aligned; else DIN_E_ARG.  Forward 1 launch, backward 2; deterministic, fp32.
 * ---------------------------------------------------------------------------------------------- */
int din_lstm_fwd(const float* pre, const float* w_hh, int rows, int steps, int dirs, int hidden, float* h_out, float* gates, float* cells,
                 void* stream);
int64_t din_lstm_bwd_workspace(int rows, int dirs, int hidden);
int din_lstm_bwd(const float* g_out, const float* gates, const float* cells, const float* w_hh, int rows, int steps, int dirs, int hidden,
                 float* d_pre, float* h_prev, float* ws, int64_t ws_floats, void* stream);
int din_pctdm_pool_fwd(const float* lstm_out, int g, int n, int h, float* pooled, uint8_t* winner, float* context, void* stream);
int din_pctdm_pool_bwd(const float* g_pooled, const float* g_context, const uint8_t* winner, int g, int n, int h, float* d_lstm_out,
                       void* stream);
int din_pctdm_att_fwd(const float* pooled, const float* src, const float* ctx, const float* w_e, const float* b_e, int g, int n, int h,
                      float* y, float* gamma, void* stream);
int64_t din_pctdm_att_bwd_workspace(int g, int h);
int din_pctdm_att_bwd(const float* g_y, const float* pooled, const float* src, const float* ctx, const float* w_e, const float* gamma, int g,
                      int n, int h, float* d_pooled, float* d_src, float* d_ctx, float* d_w_e, float* d_b_e, float* ws, int64_t ws_floats,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * Small helpers used by the host mirror
 * ---------------------------------------------------------------------------------------------- */
/* out = alpha*x + beta*y (fp32, elementwise) -- ratio mean / beta-weighted sum (:144-147), residual sums */
int din_axpby(const float* x, const float* y, float* out, float alpha, float beta, int64_t n, void* stream);
/* out[b,t,i,:] = i < n_per_clip[b] ? x[b,t,i,:] : 0 -- zeroes the padding actors of Collective clips so that the batched T x MAX_N grid
 * behaves like the reference's per-clip slices boxes_features_all[b, :, :N] (infer_model.py:1286-1288); its own backward */
int din_mask_actors(const float* x, const int32_t* n_per_clip, int b, int t, int n, int c, float* out, void* stream);
/* out (+)= x * scalar[idx] with a DEVICE scalar (learnable beta, :42-44,145); out[idx] += <x,y> for its gradient */
int din_scale_by_param(const float* x, const float* scalar, int idx, float* out, int accumulate, int64_t n, void* stream);
int din_dot_accum(const float* x, const float* y, float* out, int idx, int64_t n, void* stream);
/* dst[i] = (dtype)src[i] conversions between fp32 and bf16 */
int din_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);
/* NHWC(dtype, ld/coff) -> NCHW fp32 and back: API-parity views for MyVGG16/MyInception_v3 outputs */
int din_nhwc_to_nchw_f32(const void* in, int dtype, int nb, int h, int w, int c, int ld, int coff,
                         float* out, void* stream);
int din_nchw_f32_to_nhwc(const float* in, int nb, int h, int w, int c, void* out, int dtype, int ld,
                         int coff, void* stream);
/* fused Adam step over a flat fp32 parameter/gradient buffer (train_net_dynamic.py:104,224) */
int din_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);
/* The same update for a whole parameter list in ONE launch.  Device tables: ptrs [nt][4] = {p, g, m, v} addresses, sizes [nt]
 * element counts, and one (tensor, chunk index) pair per workgroup: workgroup b updates elements
 * [chunk_index[b]*chunk_elems, +chunk_elems) of tensor chunk_tensor[b]. */
int din_adam_step_multi(const uint64_t* ptrs, const int64_t* sizes, const int32_t* chunk_tensor, const int32_t* chunk_index,
                        int nchunks, int chunk_elems, float lr, float beta1, float beta2, float eps, float weight_decay,
                        int step, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Global gradient-norm clipping inside the fused Adam step (din_amd/optim.py: FusedAdam(max_grad_norm=...)).  The semantics are
 * torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) followed by torch.optim.Adam.step() -- what the reference's trainer
 * tried and left commented out (train_net_dynamic.py:222-223) -- plus one addition: a step whose norm is not finite is skipped.
 * Three launches on one stream, over the tables of din_adam_step_multi unchanged: no allocation, no synchronisation, no atomics,
 * capturable; every sum has a fixed order, so each result is a pure function of the gradient values, the tables and chunk_elems, with
 * or without the DIN_DETERMINISTIC option.  Additive: the ABI version stays 9.
 *
 * din_grad_sqnorm_multi: workgroup b writes partials[b] = sum of g[i]^2 over elements [chunk_index[b]*chunk_elems, +chunk_elems) of
 *   tensor chunk_tensor[b], g = column 1 of ptrs [nt][4].  Every element is widened to double before it is squared and the sum is
 *   kept in double (a gradient of magnitude 1e25 has a finite fp32 norm while its square overflows fp32).  g may start at any 4-byte
 *   offset: a chunk on a 16-byte boundary is read as 16-byte vectors, any other as dwords, in the same order of addition.  partials
 *   holds nchunks doubles.  nchunks == 0 returns DIN_OK without a launch.
 * din_grad_norm_finish: one workgroup adds partials[0..n) in a fixed order (the ranges of several din_grad_sqnorm_multi launches laid
 *   end to end give ONE global norm) and one thread writes state, float[8], with plain stores:
 *     [0] norm = (float)(grad_scale * sqrt(total))       -- grad_scale: the 1 / world factor the optimizer applies, so this is the
 *                                                            norm of the AVERAGED gradient; one rounding
 *     [1] coef = min(1, max_norm / (norm + 1e-6)) in fp32 -- torch's formula; 0 when norm is not finite (the step is skipped)
 *     [2] running sum of the finite norms    [3] running maximum of the finite norms    [4] steps measured
 *     [5] steps skipped (norm not finite)    [6] steps clipped (coef < 1)               [7] 0
 *   [2..6] are read, updated and written back: the caller zeroes state once and whenever it wants the running part to restart.
 *   max_norm = +infinity measures and guards without ever clipping.  n == 0 gives norm = 0, coef = 1.
 * din_adam_step_multi_clip: din_adam_step_multi with `state` as written above.  state[0] not finite: nothing is stored -- p, exp_avg
 *   and exp_avg_sq of every tensor keep their bits.  Otherwise g is multiplied by ONE factor, grad_scale * state[1], formed once in fp32
 *   (weight decay is added after it, as in torch); with state[1] == 1 every stored bit is din_adam_step_multi's.
 * DIN_E_ARG, with nothing read or written: a null table, partials (n > 0) or state; a negative count; chunk_elems <= 0; step < 1;
 *   partials not 8-byte aligned; state not 4-byte aligned; max_norm <= 0 or NaN; grad_scale not finite.
 * ---------------------------------------------------------------------------------------------- */
int din_grad_sqnorm_multi(const uint64_t* ptrs, const int64_t* sizes, const int32_t* chunk_tensor, const int32_t* chunk_index,
                          int nchunks, int chunk_elems, double* partials, void* stream);
int din_grad_norm_finish(const double* partials, int n, float grad_scale, float max_norm, float* state, void* stream);
int din_adam_step_multi_clip(const uint64_t* ptrs, const int64_t* sizes, const int32_t* chunk_tensor, const int32_t* chunk_index,
                             int nchunks, int chunk_elems, float lr, float beta1, float beta2, float eps, float weight_decay,
                             int step, float grad_scale, const float* state, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Adam with device-resident state (din_amd/optim.py: FusedAdam(capturable=True)).  din_adam_step_multi and din_adam_step_multi_clip
 * take the learning rate and the step count as host arguments and form the bias corrections on the host: a launch captured in a HIP
 * graph would replay step 1's forever.  Here both live in a small device record, so the optimizer of the reference's step
 * (train_net_dynamic.py:104,224: torch.optim.Adam, optimizer.step()) can be part of a captured training step.  Additive: ABI 9 stays.
 *   ostate: double[4], 8-byte aligned = { [0] steps taken, [1] learning rate, [2] beta1^steps, [3] beta2^steps }.  The caller
 *   initialises it ({0, lr, 1, 1} for a fresh optimizer; a resumed one uploads the powers computed in double) and may overwrite [1]
 *   between launches (an ordinary copy on the same stream).
 * din_adam_state_advance: replaces the host's `step += 1` (torch.optim.Adam's state['step']).  One workgroup, one thread: [0] += 1,
 *   [2] *= beta1, [3] *= beta2, in fp64.  With a clip_state (din_grad_norm_finish's float[8]) whose norm [0] is not finite nothing is
 *   written: a skipped step does not count, and the next step's bias correction is that of the un-advanced count.
 * din_adam_step_multi_dev: din_adam_step_multi with lr = (float)ostate[1], and the bias corrections (float)(1 - ostate[2]) and
 *   (float)sqrt(1 - ostate[3]) formed in fp64 and rounded once.  clip_state == NULL: the gradient is multiplied by grad_scale.
 *   Otherwise as din_adam_step_multi_clip: ONE factor grad_scale * clip_state[1], and no store at all when clip_state[0] is not
 *   finite.  The update loop is the one the two other launches run.  Launch it AFTER din_adam_state_advance (steps taken >= 1).
 * Both: plain vector stores, no atomics, no allocation, no synchronisation, capturable.  DIN_E_ARG, with nothing read or written: a
 *   null table or ostate; ostate not 8-byte aligned; clip_state not 4-byte aligned; a negative count; chunk_elems <= 0; a beta of the
 *   advance outside [0, 1); grad_scale not finite.
 * ---------------------------------------------------------------------------------------------- */
int din_adam_state_advance(double* ostate, const float* clip_state, float beta1, float beta2, void* stream);
int din_adam_step_multi_dev(const uint64_t* ptrs, const int64_t* sizes, const int32_t* chunk_tensor, const int32_t* chunk_index,
                            int nchunks, int chunk_elems, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                            const double* ostate, const float* clip_state, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Frame cache: n byte-row copies in one launch (din_amd/frame_cache.py).  Replaces, from the second epoch on, what the reference does
 * for every frame of every epoch: decode + resize + stack on the host (volleyball.py:223-275) and a blocking upload of the batch
 * (train_net_dynamic.py:174) -- decoded uint8 frames stay in HBM slots and a batch is gathered from them.
 * src, dst: DEVICE arrays of n device addresses; row i copies `bytes` bytes from src[i] to dst[i]; src[i] == 0 leaves row i alone.
 * Rows may start at any byte alignment and `bytes` may be any value >= 0 (16-byte vectors wherever src[i] and dst[i] agree mod 16,
 * narrower vectors otherwise, single bytes for head and tail).  Sources may repeat; destinations must not overlap each other or any
 * source.  One plain launch over (row, segment) on `stream`: no allocation, no synchronisation, capturable.  n == 0 or bytes == 0
 * returns DIN_OK without a launch; n < 0, bytes < 0 or a null table with n > 0 returns DIN_E_ARG before any launch.  Additive: the ABI
 * version stays 9.
 * ---------------------------------------------------------------------------------------------- */
int din_copy_rows_u8(const uint64_t* src, const uint64_t* dst, int n, int64_t bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Flip augmentation (cfg.flip_prob, din_amd/frame_cache.py): the same gather with some rows mirrored left-right on their way.
 * Row i is `lines` lines of `width` bytes (a uint8 [3, H, W] frame: lines = 3 * H, width = W).  src, dst: as for din_copy_rows_u8;
 * src[i] == 0 leaves row i alone.  flip: a DEVICE array of n int64 flags (int64 so that they travel in the buffer of the address
 * tables), or null: all zero.
 *   flip[i] == 0   row i is copied exactly as din_copy_rows_u8 copies lines * width bytes;
 *   flip[i] != 0   dst[i][l * width + x] = src[i][l * width + width - 1 - x] for every line l and column x.
 * Any width, any alignment; where width is a multiple of 16 and both addresses of a row are 16-byte aligned (every real frame) a mirrored
 * row moves as 16-byte vectors whose bytes are reversed in registers, otherwise byte by byte.  Every access lies inside the two ranges
 * of its row.  Sources may repeat; destinations must not overlap each other or any source -- a mirrored row in particular must NOT be
 * written over its own source (the copy is not an in-place reversal).  One plain launch over (row, whole-line segment) items on
 * `stream`: no allocation, no synchronisation.  n == 0 or lines * width == 0 returns DIN_OK without a launch; a negative n, lines or
 * width, or a null src or dst with n > 0, returns DIN_E_ARG before any launch.  Additive: the ABI version stays 9.
 * ---------------------------------------------------------------------------------------------- */
int din_copy_rows_u8_flip(const uint64_t* src, const uint64_t* dst, const int64_t* flip,
                          int n, int64_t lines, int64_t width, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Colour jitter (cfg.color_jitter, din_amd/frame_cache.py): the same gather with drawn rows going through Pillow's colour enhancers on
 * their way -- the two entry points below.  Additive: the ABI version stays 9.
 *
 * What they replace: PIL.ImageEnhance.Contrast, .Brightness and .Color (Pillow: ImageEnhance.py, Image.blend), applied in that order to
 * a decoded uint8 RGB frame -- what a loader of the reference's kind (volleyball.py:223-275 decodes with Pillow) would do on the host
 * between decode and stack, once per frame and epoch.  Here the frames stay as decoded in their HBM slots and the three stages are a
 * per-pixel function applied inside the launch that builds the batch.  The results are Pillow's, byte for byte.
 *
 * A row is a uint8 [3, height, width] frame: three planes R, G, B of `height` lines of `width` bytes.
 *   L(r, g, b)      = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16, in integers          (Pillow's "L" conversion);
 *   blend(d, v, f)  = t = (float)d + f * ((float)v - (float)d) in fp32, multiply and add rounded separately; t <= 0 gives 0,
 *                     t >= 255 gives 255, anything else is truncated towards zero               (Image.blend outside [0, 1]);
 *   S               = the sum of L over the height * width pixels of the row AS STORED (before any stage);
 *   mean            = (2 * S + height * width) / (2 * height * width) in integer division      (= int(S / (height * width) + 0.5)).
 * With the row's factors (c, b, s) -- contrast, brightness, saturation, fp32 -- every pixel goes through
 *   1. contrast     each of r, g, b becomes blend(mean, v, c);
 *   2. brightness   each becomes blend(0, v, b);
 *   3. saturation   with g = L of the pixel after stages 1 and 2, each becomes blend(g, v, s);
 * every stage produces uint8.  A stage whose factor is exactly 1.0f is the identity and is skipped.
 *
 * Work items: a row is cut at whole image lines into "line groups" of LPS = max(1, 8192 / width) lines (integer division), the
 * same lines in all three planes; SEGS(height, width) = ceil(height / LPS) groups per row.  Both launches walk (row, line group) items
 * block-strided behind at most 4096 workgroups; both derive SEGS by this one rule, and so does the caller that sizes `partials`.
 * ---------------------------------------------------------------------------------------------- */

/* ------------------------------------------------------------------------------------------------
 * The grey sums of n rows, by line group (the first half of PIL.ImageEnhance.Contrast: the mean of image.convert("L")).
 * src: a DEVICE array of n device addresses of [3, height, width] uint8 rows; src[i] == 0 leaves the partials of row i alone.
 * partials: DEVICE uint32 [n * SEGS(height, width)]; partials[i * SEGS + g] = the sum of L over the pixels of line group g of row i,
 * ONE plain store per item: no atomics, nothing for the caller to clear.  Integer sums: the result does not depend on any order.
 * Rows may start at any byte alignment (16-byte loads where width and the address are multiples of 16, single bytes otherwise).
 * One plain launch on `stream`, capturable.  n == 0 or height * width == 0 returns DIN_OK without a launch.  DIN_E_ARG before any
 * launch: a null src or partials with work to do; a negative n, height or width; height * width that overflows or is >= 2^24 (a
 * partial, and the whole row's sum, must fit 32 bits with room to spare).
 * ---------------------------------------------------------------------------------------------- */
int din_rows_gray_partials(const uint64_t* src, uint32_t* partials, int n, int64_t height, int64_t width, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The frame gather of din_copy_rows_u8_flip with row i transformed by factors[3 * i .. 3 * i + 2] = (contrast, brightness,
 * saturation) on its way, as defined above (PIL.ImageEnhance.Contrast, then .Brightness, then .Color).
 * src, dst: DEVICE arrays of n device addresses of [3, height, width] uint8 rows; src[i] == 0 leaves row i alone.  flip: DEVICE int64
 * [n] or null (all zero); where flip[i] != 0 every line of row i is written in reverse byte order, jittered or not -- a batch that is
 * both mirrored and jittered is still one gather launch.  factors: DEVICE fp32 [3 * n], finite.  partials: what din_rows_gray_partials
 * wrote for the SAME src, n, height and width, earlier on the same stream; each workgroup adds its row's SEGS partials (integers, served
 * from L2) to S.  Only rows with a contrast factor other than 1 read them.
 * A row whose three factors are all exactly 1.0f is copied (or mirrored) exactly as din_copy_rows_u8_flip does it; factors == null and
 * partials == null together mean that for every row.  Where width and both addresses of a row are multiples of 16 (every real frame) a
 * jittered row moves as 16-byte vectors, two loads per plane in flight before the first store; any other width or alignment goes byte
 * by byte.  Every access lies inside the two ranges of its row; all stores are plain vector stores, no atomics: capturable.  Sources
 * may repeat; a destination row must not overlap any source or any other destination.
 * n == 0 or height * width == 0 returns DIN_OK without a launch.  DIN_E_ARG before any launch: a null src or dst with work to do; a
 * negative n, height or width; height * width that overflows or is >= 2^24; factors null with partials non-null, or the reverse.
 * ---------------------------------------------------------------------------------------------- */
int din_copy_rows_u8_jitter(const uint64_t* src, const uint64_t* dst, const int64_t* flip, const float* factors,
                            const uint32_t* partials, int n, int64_t height, int64_t width, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The labels of the mirrored clips, in place, one launch for a batch.  rows = B * T frames; flip: the int64 flags of
 * din_copy_rows_u8_flip, one per row.  boxes: fp32 [rows, n, 4] in feature px (x1, y1, x2, y2), or null.  For a flagged row r and box
 * j < (n_valid ? n_valid[r] : n): (x1, y1, x2, y2) -> (width - x2, y1, width - x1, y2), each new coordinate ONE fp32 subtraction (RoIAlign
 * samples continuous coordinates with pixel centres at +0.5, so column x of a map `width` wide mirrors to width - x).  Boxes at
 * j >= n_valid[r] (the zero padding of the collective set) and unflagged rows are untouched.  activities: int64 [rows], or null.  For a
 * flagged row, a = label_map[a] where label_map (DEVICE int64 [classes]) is non-null and 0 <= a < classes; otherwise a is unchanged.
 * No allocation, no synchronisation.  rows == 0, or nothing to do (no boxes or n == 0, and no activities or no label_map), returns
 * DIN_OK without a launch; a negative rows, n or classes, or null flags where there is work, returns DIN_E_ARG before any launch.
 * Additive: the ABI version stays 9.
 * ---------------------------------------------------------------------------------------------- */
int din_flip_clip_labels(float* boxes, int64_t* activities, const int64_t* flip, const int32_t* n_valid,
                         const int64_t* label_map, int rows, int n, float width, int classes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Box-feature cache: the one launch of a frozen-backbone step (din_amd/feature_cache.py).  The trunk of the reference
 * (infer_model.py:152-184: backbone, multi-scale fuse, RoIAlign) is, with a frozen backbone, a pure function of a frame and its boxes;
 * its fp32 output row stays in an HBM slot and this launch lets a step skip the trunk for every frame that has one.
 * src, dst, keep, ref_boxes: DEVICE arrays of n device addresses (keep and ref_boxes may be null: all zero).  Row i:
 *   src[i] == 0        the row is left alone: nothing is written, flags[i] is untouched;
 *   otherwise          row_bytes bytes go from src[i] to dst[i];
 *   keep[i] != 0       the same bytes (the source is read once) are also written to keep[i], and the box_bytes bytes at
 *                      boxes + i * box_bytes to keep[i] + row_bytes -- the slot's trailer: the boxes the features were computed for;
 *   ref_boxes[i] != 0  the box_bytes bytes there are compared bytewise with boxes + i * box_bytes; on any difference flags[i] = 1 is
 *                      written with a plain store.  0 is never written: the caller clears flags at the start of a pass.
 * Every address in the tables, boxes, row_bytes and box_bytes are multiples of 16 (all traffic is 16-byte vectors); a row holding an
 * address that is not, or a zero dst[i], is left alone like a row with src[i] == 0.  Sources may repeat; destinations and slots must not
 * overlap each other, any source, or any ref_boxes row of the same launch.  One plain launch over (row, segment) items of
 * DIN_FEAT_ROWS_SEGMENT bytes on `stream`: no allocation, no synchronisation, no atomics, capturable.  n == 0 returns DIN_OK without a
 * launch.  DIN_E_ARG before any launch: n, row_bytes or box_bytes negative; row_bytes, box_bytes or `boxes` not a multiple of 16; a null
 * src or dst with n > 0; a null boxes or flags with a non-null keep or ref_boxes.  Additive: the ABI version stays 9.
 * ---------------------------------------------------------------------------------------------- */
#define DIN_FEAT_ROWS_SEGMENT 16384
int din_feat_rows(const uint64_t* src, const uint64_t* dst, const uint64_t* keep, const uint64_t* ref_boxes,
                  const void* boxes, uint8_t* flags, int n, int64_t row_bytes, int box_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The same launch over slots that hold bf16 rows (cfg.feature_cache_dtype = 'bf16', din_amd/feature_cache.py): with the backbone in
 * bf16 the embedding GEMM that reads feats (infer_model.py:184) multiplies bf16 operands, so the row is stored already rounded -- half
 * the bytes per frame, and no cast pass over feats in a cached step.  Rows are row_elems bf16 values at dst[i] and keep[i].
 * src, dst, keep, ref_boxes, boxes, flags, box_bytes: as for din_feat_rows with row_bytes = 2 * row_elems (the trailer is at
 * keep[i] + 2 * row_elems).  src_f32: a DEVICE array of n entries, or null: all zero.  Row i with src[i] != 0:
 *   src_f32[i] != 0    src[i] addresses row_elems FP32 values (the row the trunk just computed): each is read once and rounded once to
 *                      bf16, round-to-nearest-even (the gfx950 hardware conversion: NaN stays NaN), and the rounded row goes to dst[i]
 *                      and, where keep[i] != 0, to keep[i], followed there by the boxes;
 *   src_f32[i] == 0    src[i] addresses row_elems bf16 values (a slot): copied unchanged, exactly din_feat_rows.
 * Every address in the tables, `boxes` and box_bytes are multiples of 16 and row_elems is a multiple of 8; a row holding an address that
 * is not, or a zero dst[i], is left alone like a row with src[i] == 0.  Overlap rules, the (row, segment) items of
 * DIN_FEAT_ROWS_SEGMENT bytes of the DESTINATION row (8192 values), the single plain launch on `stream` -- no allocation, no
 * synchronisation, no atomics, capturable -- and n == 0 are din_feat_rows's.  DIN_E_ARG before any launch: n, row_elems or box_bytes
 * negative; row_elems not a multiple of 8; box_bytes or `boxes` not a multiple of 16; a null src or dst with n > 0; a null boxes or
 * flags with a non-null keep or ref_boxes.  Additive: the ABI version stays 9.
 * ---------------------------------------------------------------------------------------------- */
int din_feat_rows_bf16(const uint64_t* src, const uint64_t* dst, const uint64_t* keep, const uint64_t* ref_boxes,
                       const uint64_t* src_f32, const void* boxes, uint8_t* flags, int n, int64_t row_elems, int box_bytes,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIN_HIP_H */
