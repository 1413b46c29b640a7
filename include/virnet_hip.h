/*
 * virnet_hip.h -- C ABI of the MI355X (gfx950) kernels behind VIRNet's convolutional forward.
 *
 * The reference (zsyOAOA/VIRNet) is pure Python on PyTorch: it has no FFI, plugin or operator
 * registry.  Its boundary for this path is the nn.Module surface of networks/VIRNet.py
 * (VIRAttResUNet.forward :42-46, VIRAttResUNetSR.forward :80-97) and the arithmetic sits in
 * torch.nn.functional call sites.  Each entry point below therefore cites the reference CALL SITE
 * (file:line under /root/reference) whose arithmetic it replaces; the modules under virnet_amd/networks/ is the
 * Python host side that mirrors the reference classes and binds these symbols through ctypes
 * (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless stated otherwise; no torch types cross the ABI
 *   - activations between kernels are NHWC fp32 ("pixel records"), channel count a multiple of 16
 *   - images enter and leave as NCHW fp32 exactly as the reference modules receive/return them
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous
 *   - return value: 0 on success, non-zero on error; virnet_last_error() gives the message
 */
#ifndef VIRNET_HIP_H
#define VIRNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): round 4's additions -- virnet_t_emit / virnet_knet_layer, the emitting and persistent entry points, the convT weight image
 * that keeps cin when cin % 32 == 0 -- were shipped under version 1; a stale library now fails the version check instead of an
 * AttributeError / a mis-sized packing.
 * 4 (round 6): virnet_conv_wx4_last_plan; the packed entry image (virnet_pack_entry_weight / virnet_entry_weight_floats) carries a four-word
 * trailer {cin, k-steps per row, n_pad, tag} that virnet_conv_entry's kernel checks against the launch (a mismatch gives NaN).
 * 5: gradients with respect to the input image -- virnet_image_grad / virnet_image_grad_desc, virnet_conv_head_s4_dgrad.
 * (still 5): the device-side metrics -- virnet_quantize_u8, virnet_rgb2y_u8, virnet_psnr_ssim_workspace_bytes, virnet_psnr_ssim.  Purely
 * additive (new symbols, no struct or existing signature changed), so a caller built against the earlier version 5 keeps working and the
 * number is not bumped; a library WITHOUT them fails the binding's symbol check (virnet_amd/_native.py) by name.
 * (still 5): virnet_conv_plan_query / virnet_conv_launch -- the launch rules of the split-fp16 conv hosts as a query; additive as above.
 * (still 5): the SISR objective -- virnet_sisr_head_*, virnet_sisr_hr_*, virnet_sisr_lr_*, virnet_sisr_finish; additive as above.
 * (still 5): virnet_conv_wgrad_f16_plan_query -- the split-K plan of the f16-pipe weight gradients as a query; additive as above.
 * (still 5): the JPEG round trip -- virnet_jpeg_workspace_bytes, virnet_jpeg_roundtrip; additive as above.
 * (still 5): the gradient buckets -- virnet_gradsync_pack, virnet_gradsync_unpack, virnet_gradsync_launches; additive as above.
 * (still 5): tiled whole-image restoration -- virnet_tile_gather, virnet_tile_blend; additive as above.
 * (still 5): training previews -- virnet_preview_grid_workspace_bytes, virnet_preview_grid, virnet_kernel_from_kinfo; additive as above. */
#define VIRNET_ABI_VERSION 5

int virnet_abi_version(void);
const char* virnet_last_error(void);
/* number of visible HIP devices, or -1 when the runtime cannot be initialised */
int virnet_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * Weight packing.  Reference layouts in, MFMA-fragment ("stage") layout out.
 *   kind 0: nn.Conv2d weight  [Cout][Cin][KS][KS]            (AttResUNet.py:43,46,67,117,139; DnCNN.py:22-29;
 *                                                             KNet.py:32,34,49)
 *   kind 1: nn.ConvTranspose2d(k=2,s=2) weight [Cin][Cout][2][2] (AttResUNet.py:80), packed as the equivalent
 *           1x1 GEMM to N = 4*Cout columns ordered (a*2+b)*Cout + co
 * `cin_pad` (multiple of 16) and `n_pad` (multiple of 32*nrep) give the zero-padded GEMM extents; `nrep` is the
 * number of 32-column blocks one workgroup owns (see virnet_conv_plan).
 * ---------------------------------------------------------------------------------------------- */
/*   kind 2: the input-gradient ("dgrad") weights of a 3x3 conv, W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx]: pass the forward
 *           OIHW tensor, cout/cin are the FORWARD counts; the packed GEMM has cin rows (n_pad covers cin) and cout_fwd
 *           contraction channels (cin_pad covers cout).  Used with stride 1 (a stride-2 conv's dgrad runs on the zero-stuffed
 *           gradient, virnet_zero_stuff2).
 *   kind 3: dgrad weights of the 2x2/s2 transposed conv: a 1x1 GEMM over the space-to-depth gradient
 *           (virnet_space_to_depth2): W'[ci][ab*cout+co] = Wt[ci][co][a][b]; n_pad covers cin, cin_pad covers 4*cout. */
size_t virnet_packed_weight_floats(int ks, int cin_pad, int n_pad);
int virnet_pack_weight(const float* w, int kind, int cout, int cin, int ks, int cin_pad, int n_pad, int nrep,
                       float* packed, void* stream);

/* Tile plan chosen by the library for one conv shape (so the host can pack with the right nrep). */
typedef struct virnet_conv_plan {
  int nrep;    /* 32-column blocks per workgroup (GEMM-N block = 32*nrep) */
  int n_pad;   /* padded GEMM-N extent */
  int cin_pad; /* padded Cin (multiple of 16) */
} virnet_conv_plan;
/* ks in {1,3}; stride in {1,2}; gemm_n = Cout (conv) or 4*Cout (transposed conv) */
int virnet_conv_get_plan(int ks, int stride, int cin, int gemm_n, virnet_conv_plan* plan);

/* ------------------------------------------------------------------------------------------------
 * The MFMA implicit-GEMM convolution (v_mfma_f32_32x32x2_f32, exact fp32).
 * Replaces: AttResBlock.conv1/conv2 (AttResUNet.py:55,58 with the residual add :59), DownBlock.downsampler
 * (AttResUNet.py:67), UpBlock.upsampler + bridge add (AttResUNet.py:84-87), AttResUNet.head/tail (:153-155,:173),
 * DnCNN.conv1/mid_layer/conv_last (DnCNN.py:38-41), RB_Layer convs and KernelNet.tail conv (KNet.py:32-34,49).
 * ---------------------------------------------------------------------------------------------- */
enum { VIRNET_EPI_NHWC = 0, VIRNET_EPI_CONVT = 1, VIRNET_EPI_NCHW = 2 };
enum { VIRNET_NCHW_PLAIN = 0, VIRNET_NCHW_ADD = 1, VIRNET_NCHW_EXPCLAMP = 2 };

typedef struct virnet_conv_desc {
  const float* x;      /* NHWC [n][h][w][cin_pad] */
  const float* wpack;  /* from virnet_pack_weight */
  const float* bias;   /* [cout] or NULL */
  const float* res;    /* EPI_NHWC: NHWC [n][oh][ow][cout] residual (AttResUNet.py:59) or NULL
                          EPI_CONVT: NHWC [n][2h][2w][cout] bridge (AttResUNet.py:87) or NULL
                          EPI_NCHW : NCHW [n][cout][crop_h][crop_w] (the `+ x_in` of AttResUNet.py:173) or NULL */
  const float* mul;    /* [n][cout] SFT scale applied to y_act (AttResUNet.py:57-58) or NULL (=1); mul and add are given together */
  const float* add;    /* [n][cout] SFT shift applied to y_act or NULL (=0), with mul */
  const float* mask;   /* EPI_NHWC only, backward passes: tensor of the output's shape; acc is multiplied by lrelu'(mask) =
                          (mask > 0 ? 1 : mask_slope) BEFORE res is added (d_pre = d_act * lrelu'(saved), AttResUNet.py:55,58) */
  const float* in_mul; /* [n][cin_pad] SFT scale applied to x while it is staged (AttResUNet.py:54-55) or NULL (=1) */
  const float* in_add; /* [n][cin_pad] SFT shift applied to x while it is staged or NULL (=0) */
  float* y_raw;        /* conv + bias (+res); NULL = not stored */
  float* y_act;        /* leaky_relu(y_raw*mul+add, slope); NULL = not stored (EPI_NHWC / EPI_CONVT only) */
  int n, h, w;         /* input batch / spatial size */
  int cin_pad;         /* channels of x (multiple of 16) */
  int cout;            /* real output channels (EPI_CONVT: channels of the up-sampled tensor) */
  int n_pad;           /* padded GEMM-N extent used when packing */
  int nrep;            /* from the plan used when packing */
  int ks, stride;      /* {3,1}: s1 or s2, pad 1 ; {1,1}: pointwise */
  int epi;             /* VIRNET_EPI_* */
  int nchw_op;         /* VIRNET_NCHW_* (EPI_NCHW only) */
  int crop_h, crop_w;  /* EPI_NCHW: stored extent (<= oh, ow) */
  int res_sf;          /* EPI_NCHW + VIRNET_NCHW_ADD: res is [n][cout][crop_h/res_sf][crop_w/res_sf] and is read through a
                          nearest x res_sf up-sampling (the x_up of VIRNet.py:83 added at AttResUNet.py:173); 0/1 = none */
  int in_act;          /* 1: the conv consumes leaky_relu(x*in_mul+in_add, in_slope) -- the pre-activation of AttResUNet.py:55 --
                          applied to the pixels on their way into LDS; padding stays zero AFTER the activation. 0: plain x */
  float in_slope;      /* LeakyReLU slope of the input activation */
  float slope;         /* LeakyReLU slope of y_act */
  float mask_slope;    /* slope of the LeakyReLU whose derivative `mask` selects */
  float clamp_lo, clamp_hi; /* VIRNET_NCHW_EXPCLAMP: y = exp(clamp(v, lo, hi))  (VIRNet.py:43) */
} virnet_conv_desc;

int virnet_conv_mfma(const virnet_conv_desc* d, void* stream);
/* Which instantiation virnet_conv_mfma would launch for `d`: out = {KS, STRIDE, MREP, NREP} of
 * conv_mfma_kernel<KS,STRIDE,MREP,NREP> (the name rocprofv3 reports).  Used by bench.py to attribute event timings. */
int virnet_conv_mfma_variant(const virnet_conv_desc* d, int out[4]);
/* The whole instantiation: out = {KS, STRIDE, MREP, NREP, NW} of conv_mfma_kernel<KS,STRIDE,MREP,NREP,NW> (NW = waves per workgroup,
 * 4 or 8), from the same tile rule as the launch -- under VIRNET_FORCE_MREP / _NREP / _NW as they stand at the call.  Needs no device;
 * of the descriptor only nrep >= 1 and stride >= 1 are checked (virnet_conv_mfma_check does the rest). */
int virnet_conv_mfma_tile(const virnet_conv_desc* d, int out[5]);
/* Every check virnet_conv_mfma makes of a descriptor, and nothing else: no device, no launch, no pointer is followed.  0, or non-zero
 * with virnet_last_error() naming the check that refused it. */
int virnet_conv_mfma_check(const virnet_conv_desc* d);

/* ------------------------------------------------------------------------------------------------
 * The same stride-1 3x3 convolution in Winograd F(2x2,3x3) form (16 instead of 36 multiplies per 2x2 output tile and channel
 * pair; fp32 on v_mfma_f32_32x32x2_f32).  Call sites: AttResBlock.conv1/conv2 (AttResUNet.py:55,58 + residual :59), DnCNN
 * mid_layer (DnCNN.py:25-28,39-40) and their input-gradient GEMMs in the training step.  Takes the SAME descriptor as
 * virnet_conv_mfma with ks = 3, stride = 1, epi = VIRNET_EPI_NHWC, cout a multiple of 32 (n_pad = cout; nrep is ignored) and
 * `wpack` from virnet_pack_wino_weight: U = G g G^T per channel pair, [cout/32][cin_pad/4][16 positions][2][32][2] floats.
 * `dgrad` = 1 packs the input-gradient GEMM of the layer (W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx]; pass the forward OIHW tensor
 * and the FORWARD cout/cin; n_pad then covers cin and cin_pad covers cout, as for kind 2 of virnet_pack_weight).
 * ---------------------------------------------------------------------------------------------- */
size_t virnet_wino_weight_floats(int cin_pad, int n_pad);
int virnet_pack_wino_weight(const float* w_oihw, int dgrad, int cout, int cin, int cin_pad, int n_pad, float* packed, void* stream);
int virnet_conv_wino(const virnet_conv_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The same stride-1 3x3 convolution on the f16 matrix pipe with SPLIT fp32 operands (csrc/conv_f16.hip): every fp32 weight and
 * activation is written exactly as hi + lo in fp16 and w*x is evaluated as w_lo*x_hi + w_hi*x_lo + w_hi*x_hi on
 * v_mfma_f32_32x32x16_f16 with fp32 accumulation -- fp32-class results (measured error vs fp64 no larger than the fp32 MFMA
 * chain's, profiles/r02_probes.md) at 3/16 of the fp32 matrix pipe's cycles.  Call sites as virnet_conv_wino: AttResBlock.conv1/
 * conv2 (AttResUNet.py:55,58 + residual :59), DnCNN mid_layer (DnCNN.py:25-28,39-40), RB_Layer convs (KNet.py:32,34) and their
 * input-gradient GEMMs.  Takes the SAME descriptor as virnet_conv_mfma with ks = 3, stride = 1, epi = VIRNET_EPI_NHWC, cout a
 * multiple of 32 (n_pad = cout; nrep is ignored) and `wpack` from virnet_pack_f16_weight: n_pad inverse row scales (fp32) followed
 * by the split image [n_pad/32][cin_pad/16][9 taps, column-major][hi|lo][64 lanes][8 x fp16].  Weights are scaled per output
 * channel by a power of two (exact).  `dgrad` as for virnet_pack_wino_weight.  Activations must stay below 65504 in magnitude.
 * ---------------------------------------------------------------------------------------------- */
size_t virnet_f16_weight_floats(int cin_pad, int n_pad);
int virnet_pack_f16_weight(const float* w_oihw, int dgrad, int cout, int cin, int cin_pad, int n_pad, float* packed, void* stream);
int virnet_conv_f16(const virnet_conv_desc* d, void* stream);
/* The other two dense layers of the U-Net on the same pipe, through virnet_conv_f16:
 *   - ks = 3, stride = 2, epi = VIRNET_EPI_NHWC (DownBlock.downsampler, AttResUNet.py:67,74): `wpack` from virnet_pack_f16_weight,
 *     bias / single-store epilogue only (csrc/conv_f16_s2.hip);
 *   - ks = 1, epi = VIRNET_EPI_CONVT (UpBlock.upsampler + bridge add, AttResUNet.py:80,84-87): `wpack` from
 *     virnet_pack_f16_convt_weight (the IOHW [cin][cout][2][2] tensor as the pointwise GEMM to rows (a*2+b)*cout + co, contraction
 *     kept as is when cin is a multiple of 32 -- K then runs in 2-chunk stages with two workgroups per CU -- else zero-padded to a
 *     multiple of 48: virnet_f16_convt_weight_floats sizes it), n_pad = 4*cout, bias + `res` (bridge) / single-store epilogue (csrc/conv_f16_pw.hip). */
/* bf16-OPERAND variant of the stride-1 3x3 NHWC convolution (BASELINE configs[4]'s training precision; reduced accuracy, ~4e-3 per
 * operand): ONE v_mfma_f32_32x32x16_bf16 per k-step, operands rounded to bf16 (activations while staged, weights when packed), fp32
 * accumulation, bias / mask / residual / activation in fp32.  Same descriptor; `wpack` from virnet_pack_bf16_weight (same size and
 * layout as the f16 image: virnet_f16_weight_floats). */
int virnet_pack_bf16_weight(const float* w_oihw, int dgrad, int cout, int cin, int cin_pad, int n_pad, float* packed, void* stream);
int virnet_conv_bf16(const virnet_conv_desc* d, void* stream);
size_t virnet_f16_convt_weight_floats(int cin, int cout);
int virnet_pack_f16_convt_weight(const float* w_iohw, int cout, int cin, float* packed, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The same stride-1 3x3 NHWC convolution in Winograd F(4,3) form ALONG X (direct along y) on the f16 matrix pipe with split fp32
 * operands (csrc/conv_f16_wx4.hip): 6 transform positions x 3 row taps = 18 k-steps per 4 output pixels instead of 36, i.e. 1.5
 * executed FLOP per algorithmic FLOP instead of conv_f16's 3, same three-product fp32-class arithmetic per position product.
 * Call sites as virnet_conv_f16: AttResBlock.conv1/conv2 (AttResUNet.py:55,58 + residual :59), DnCNN mid_layer (DnCNN.py:25-28,39-40)
 * and their input-gradient GEMMs.  SAME descriptor (ks = 3, stride = 1, epi = VIRNET_EPI_NHWC, cout % 32 == 0, n_pad = cout) with
 * `wpack` from virnet_pack_wx4_weight: n_pad inverse row scales followed by U[dy][j] = sum_b G[j][b] w[dy][b] (formed in fp64) as
 * the split image [n_pad/32][cin_pad/16][6 positions][3 dy][hi|lo][64 lanes][8 x fp16].  Accuracy: the Winograd transform adds
 * rounding relative to the largest magnitude inside a 6-pixel input window (not per output): whole denoise-syn network 1.1e-5 max-abs
 * against fp64 (conv_f16 8.0e-6, fp32 direct 8.9e-6).  Transformed activations must stay below 65504 (|x| < 6.5e3).
 * ---------------------------------------------------------------------------------------------- */
size_t virnet_wx4_weight_floats(int cin_pad, int n_pad);
int virnet_pack_wx4_weight(const float* w_oihw, int dgrad, int cout, int cin, int cin_pad, int n_pad, float* packed, void* stream);
int virnet_conv_wx4(const virnet_conv_desc* d, void* stream);
/* What the calling thread's most recent virnet_conv_wx4 / virnet_conv_wx4_emit call launched (the library picks the tile form per launch
 * size, csrc/conv_f16_wx4.hip): out[0] = tile rows of its first launch (16: conv_f16_wx4.hip / conv_f16_wx4p.hip, 8: conv_f16_wx4h.hip),
 * out[1] = 1 when that launch was the persistent form (VIRNET_WX4_PERSIST=1), out[2] = 32-channel slabs per workgroup, out[3] = launches. */
void virnet_conv_wx4_last_plan(int* out4);
/* REDUCED-PRECISION variant of virnet_conv_wx4 for inference (csrc/conv_f16_wx4x1.hip; VIRNET_CONV_FORM=wx4x1): the same Winograd form
 * with ONE v_mfma_f32_32x32x16_f16 per position product instead of three -- 18 MFMAs per 4 output pixels.  Call sites as virnet_conv_wx4
 * (AttResBlock.conv1/conv2, AttResUNet.py:55,58-59; DnCNN mid_layer, DnCNN.py:25-28; KNet.py:32,34), forward only: no T emission, no
 * input-gradient use.  SAME descriptor and the SAME `wpack` (virnet_pack_wx4_weight): only the image's hi pieces are read, i.e. the
 * weights are fp16(U * 2^e) with the row maximum in [8192, 16384); the activations' V = B^T x is formed in fp32 exactly as in
 * virnet_conv_wx4 and rounded ONCE to fp16 (no lo part); fp32 accumulation; inverse scale, A^T, bias, mask, residual, output SFT and
 * activation in fp32.  Accuracy: 11-bit operands -- whole denoise-syn network 1.2e-2 max-abs on mu against fp64 (virnet_conv_bf16's
 * arithmetic 5.8e-2, virnet_conv_wx4 1.2e-5; tools/numerics_gate.py).  Same range limit and range flag as virnet_conv_wx4 (transformed
 * magnitude below 65520).  One tile form (16 x 32 pixels, 8 waves), slabs per workgroup by launch size (VIRNET_PLAN_WX4X1). */
int virnet_conv_wx4x1(const virnet_conv_desc* d, void* stream);

/* One kernel launch of a split-fp16 convolution host: `groups` workgroup columns of ng * nrep 32-channel slabs each, starting at slab
 * `slab_base`.  form: which kernel file; rows: tile height in output rows (0: the pointwise transposed form); variant: the direct kernel's
 * MREP (8- / 4-row tiles) or the transposed conv's chunks per stage (KS), else 0; persistent: 1 for conv_f16_wx4p.hip. */
enum { VIRNET_LAUNCH_WX4 = 0, VIRNET_LAUNCH_WX4H = 1, VIRNET_LAUNCH_WX4P = 2, VIRNET_LAUNCH_F16 = 3, VIRNET_LAUNCH_S2 = 4, VIRNET_LAUNCH_CONVT = 5,
       VIRNET_LAUNCH_WX4X1 = 6 };
typedef struct virnet_conv_launch {
  int form, rows, ng, nrep, variant, slab_base, groups, persistent;
} virnet_conv_launch;
/* family: whose rules -- virnet_conv_wx4 (with emit_rows 8 / 16: virnet_conv_wx4_emit), virnet_conv_f16 (stride 1, stride 2 or transposed
 * by the descriptor; emit_rows 8: virnet_conv_f16_emit), virnet_conv_bf16, virnet_conv_f16_entry (the descriptor's own checks only),
 * virnet_conv_wx4x1 (no emission). */
enum { VIRNET_PLAN_WX4 = 0, VIRNET_PLAN_F16 = 1, VIRNET_PLAN_BF16 = 2, VIRNET_PLAN_F16_ENTRY = 3, VIRNET_PLAN_WX4X1 = 4 };
/* What virnet_conv_wx4 / virnet_conv_f16 (stride 1, stride 2, transposed) would launch for this descriptor,
 * without launching: fills up to `cap` records and returns the number of launches (< 0: error, see
 * virnet_last_error). n_cu <= 0: the current device's CU count (256 when there is no device). Reads the same
 * knobs at the same moments as the launch functions. Pointers in `d` are only tested for NULL-ness. */
int virnet_conv_plan_query(int family, const virnet_conv_desc* d, int emit_rows, int n_cu,
                           virnet_conv_launch* out, int cap);

/* Few-output-channel exits with planar store (csrc/conv_exit.hip): AttResUNet.tail + crop + `+ x_in` (AttResUNet.py:139,173),
 * DnCNN.conv_last + exp(clamp) (DnCNN.py:29,41; VIRNet.py:43), KernelNet.tail (KNet.py:49) -- for cout * 9 <= 32 the (channel, tap) pairs
 * are the ROWS of one pointwise split-fp16 GEMM and the taps are summed afterwards: the input is read once, straight into MFMA
 * fragments (HBM-bound; algorithmic bytes n*h*w*cin_pad*4 in + 4 per output value).  `d` as for virnet_conv_f16 with epi =
 * VIRNET_EPI_NCHW (nchw_op, crop, res / res_sf, clamp honoured; in_act / in_slope optional); wpack from virnet_pack_exit_weight:
 * 32 inverse row scales, then [cin_pad/16][hi|lo][64 lanes][8 x fp16]. */
size_t virnet_exit_weight_floats(int cin_pad);
int virnet_pack_exit_weight(const float* w_oihw, int cout, int cin, int cin_pad, float* packed, void* stream);
int virnet_conv_exit(const virnet_conv_desc* d, void* stream);
/* The same launch with an ADDITIVE PARTIAL MAP: z_add [n][h][w][32] fp32 (NHWC, on the same h x w as x) holds a contribution to the
 * rows z[(c, tap)][pixel] at their true scale; the kernel forms z = A x + z_add before the taps are summed (halo pixels outside the
 * image read zeros).  cin_pad = 96 or 64, no in_act.  With virnet_compose_exit_weight this is the exit conv applied to
 * y = x + conv3x3(t; w2) + b2 without y ever being stored: z_add = conv3x3(t; wc) + bc (any conv kernel, plain NHWC store of 32 channels). */
int virnet_conv_exit_add(const virnet_conv_desc* d, const float* z_add, void* stream);
/* wc [32][cin][3][3] (OIHW, rows cout_exit*9 .. 31 zero) and bc [32] from w2 [cmid][cin][3][3], b2 [cmid] (NULL = none) and the exit
 * weight w_exit [cout_exit][cmid][3][3]: wc[c*9 + t][ci][k] = sum_m w_exit[c][m][t] * w2[m][ci][k], bc likewise from b2; accumulated in
 * fp64, rounded once.  cout_exit * 9 <= 32.  The result goes through the ordinary weight packers. */
int virnet_compose_exit_weight(const float* w2, const float* b2, const float* w_exit, int cout_exit, int cmid, int cin, float* wc, float* bc,
                               void* stream);

/* Range guard of the split-fp16 kernels (virnet_conv_f16 incl. its stride-2 / transposed forms, virnet_conv_wx4).  An operand of magnitude
 * >= 65520 (transformed magnitude for virnet_conv_wx4: up to 10x the activation) does not fit fp16: the product turns Inf / NaN, which is
 * loud in a tensor but clamped away by the exp(clamp(.)) / tanh epilogues (VIRNet.py:43, KNet.py:56-58).  Register a zeroed device int per
 * device (NULL = off); the kernels OR 1 into it when a staged operand leaves the range.  The host side (virnet_amd/engine.py) reads it at
 * the end of a forward and re-runs the image in the fp32 Winograd form.  The reference's fp32 path has no such limit. */
int virnet_set_range_flag(int* device_flag);
/* (the registration is per (device, calling host thread): forwards driven from several threads keep separate flags)
 * virnet_poison_on_flag: fills y[0..n) with NaN when *device_flag != 0 -- the last node of a replayed hipGraph (virnet_amd/graph.py), so
 * that an out-of-range forward is loud even before the host has read the flag. */
int virnet_poison_on_flag(const int* device_flag, float* y, size_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3x3 convolution to 1..4 output channels with planar store (HBM/LDS-bound VALU kernel, not MFMA work):
 * AttResUNet.tail + crop + `+ x_in` (AttResUNet.py:139,173), DnCNN.conv_last + exp(clamp) (DnCNN.py:29,41; VIRNet.py:43),
 * KernelNet.tail conv (KNet.py:49).  Weights: virnet_pack_thin_weight of the OIHW tensor.
 * ---------------------------------------------------------------------------------------------- */
typedef struct virnet_thin_desc {
  const float* x;      /* NHWC [n][h][w][c], c a multiple of 16 */
  const float* wpack;  /* [c/16][9][16][4] from virnet_pack_thin_weight */
  const float* bias;   /* [cout] or NULL */
  const float* res;    /* VIRNET_NCHW_ADD: NCHW [n][cout][crop_h/res_sf][crop_w/res_sf] */
  float* y;            /* NCHW [n][cout][crop_h][crop_w] */
  int n, h, w, c, cout;
  int crop_h, crop_w;  /* stored extent (<= h, w) */
  int op;              /* VIRNET_NCHW_* */
  int res_sf;          /* nearest up-sampling factor of res (0/1 = none) */
  float clamp_lo, clamp_hi;
} virnet_thin_desc;
size_t virnet_thin_weight_floats(int c_pad);
int virnet_pack_thin_weight(const float* w_oihw, int cout, int c, int c_pad, float* packed, void* stream);
int virnet_conv3x3_thin(const virnet_thin_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Image entry: NCHW -> 16-channel NHWC pixel records, fusing
 *   - the nearest x`sf` up-sampling of VIRNet.py:83 (sf = 1 for denoising),
 *   - the bottom/right reflect pad of utils/util_net.py:20-25 (hp >= h*sf, wp >= w*sf),
 *   - the channel concat of AttResUNet.py:153 with per-image vectors (kinfo / sqrt(sigma) repeated, VIRNet.py:89,92)
 *     and/or a per-pixel map (sigma map; VIRNet.py:44 sqrt, VIRNet.py:94 nearest x msf).
 * Channel order: [c0 image channels][ev vector channels][em map channels][zeros up to 16].
 * ---------------------------------------------------------------------------------------------- */
typedef struct virnet_pack_desc {
  const float* x;    /* NCHW [n][c0][h][w] */
  const float* vec;  /* [n][ev] or NULL */
  const float* map;  /* NCHW [n][em][mh][mw] or NULL; source pixel = (reflect(y)/msf, reflect(x)/msf) */
  float* out;        /* NHWC [n][hp][wp][16] */
  int n, c0, h, w, sf;
  int ev;
  int em, mh, mw, msf, map_sqrt;
  int hp, wp;
  int zero_pad;      /* 1: positions beyond h*sf, w*sf are zero instead of reflected (gradient records of the training step) */
} virnet_pack_desc;
int virnet_pack_input(const virnet_pack_desc* d, void* stream);
/* The same entry folded into the first convolution (AttResUNet.head AttResUNet.py:153-155, DnCNN.conv1 DnCNN.py:38): virnet_conv_f16 on
 * ONE 16-channel chunk (d->cin_pad = 16, d->h x d->w = e->hp x e->wp, plain single-store epilogue) whose staging gathers each pixel's
 * record [image | vector | map | 0] from the NCHW sources of `e` -- the packed tensor never exists (e->out is ignored; c0 + ev + em <= 8). */
int virnet_conv_f16_entry(const virnet_conv_desc* d, const virnet_pack_desc* e, void* stream);
/* Round 5: the entries as their own STORE-bound kernel (csrc/conv_entry.hip; same call sites: AttResUNet.py:153-155, DnCNN.py:38).  K is
 * walked one kernel ROW per MFMA k-step (slot j = dx * cin + ch), the B fragments are gathered from a planar fp32 copy of the input tile in
 * LDS, every output row leaves as lane-linear 1-KB stores.  cin = c0 + ev + em <= 8, cout a multiple of 32 up to 96, plain epilogue
 * (exactly one of y_raw / y_act).  Weight image: virnet_entry_weight_floats(cin, n_pad) floats from virnet_pack_entry_weight (OIHW
 * [cout][cin][3][3] in; n_pad inverse scales first).  Agrees with virnet_conv_f16_entry to fp32 rounding (other summation order). */
size_t virnet_entry_weight_floats(int cin, int n_pad);
int virnet_pack_entry_weight(const float* w, int cout, int cin, int n_pad, float* packed, void* stream);
int virnet_conv_entry(const virnet_conv_desc* d, const virnet_pack_desc* e, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training step: weight / bias gradients and the layout helpers of the input-gradient convs.
 * Input gradients themselves are virnet_conv_mfma launches with kind-2 / kind-3 packed weights and the `mask` epilogue.
 * ---------------------------------------------------------------------------------------------- */
typedef struct virnet_wgrad_desc {
  const float* x;       /* NHWC [n][h][w][cx]: the conv's forward input */
  const float* dy;      /* NHWC [n][oh][ow][cy]: gradient of the conv's output (transposed: space-to-depth gradient, cy = 4*cout) */
  const float* in_mul;  /* the forward conv's staging transform (lrelu(x*in_mul+in_add)), or NULL */
  const float* in_add;
  float* dw;            /* += : [cout][cin][ks][ks] (OIHW) or, transposed, [cin][cout][2][2]; zero it first (fp32 atomics) */
  int* counters;        /* zeroed int32 scratch, ceil(rows/32)*ceil(cin/32) entries (rows = cout, or 4*cout transposed): tile hand-out */
  int n, h, w, cx, cy;
  int cin, cout;        /* real channel counts (<= cx, cy) */
  int ks, stride;       /* {3,1} {3,2} {1,1} */
  int transposed;       /* 1: weight of ConvTranspose2d(k2,s2) */
  int in_act;
  float in_slope;
} virnet_wgrad_desc;
int virnet_conv_wgrad(const virnet_wgrad_desc* d, void* stream);
/* The same gradient for the stride-1 3x3 convs on the f16 matrix pipe (csrc/wgrad_f16.hip; backward of networks/AttResUNet.py:43,46,
 * DnCNN.py:22-29).  The contraction runs over pixels, so both operands are first re-laid CHANNEL-major as fp16 planes:
 *   T[n][h+2][ceil(c/32)][hi|lo][seg][32 ch][8 px], pixel x at index x+8 of its row, zero rows / pads around the image.
 * virnet_chsplit writes T from an NHWC fp32 tensor (c % 4 == 0), applying lrelu(x*in_mul+in_add) (the forward conv's staging transform)
 * and the hi/lo split of virnet_conv_f16 (bf16 != 0: one bf16 plane, single product); `out` holds virnet_chsplit_bytes() bytes.
 * virnet_conv_wgrad_f16: dw[cout][cin][3][3] = sum_p dy[p][co] * a[p + tap][ci] from the two T tensors (cx / cy = their stored channels);
 * the pixel range is split over workgroups whose partial sums go to `scratch` (virnet_conv_wgrad_f16_scratch_bytes() bytes, need not be
 * zeroed) and are then reduced in a fixed order: dw is overwritten, and bitwise reproducible. */
size_t virnet_chsplit_bytes(int n, int h, int w, int c);
size_t virnet_conv_wgrad_f16_scratch_bytes(int n, int h, int w, int cx, int cy);
size_t virnet_chsplit_colsum_bytes(int n, int h, int w, int c);
/* db != NULL: the bias gradient as a by-product of the dY pass, db[ch] += sum over pixels of x[..][ch] for ch < cvalid (zero db first;
 * replaces a virnet_colsum pass over the tensor); col_scratch = virnet_chsplit_colsum_bytes() bytes of per-block partial sums, which one
 * workgroup per four channels adds in a fixed order (no atomics: db is bitwise reproducible, here and in virnet_colpart_reduce). */
int virnet_chsplit(const float* x, int n, int h, int w, int c, int in_act, float in_slope, const float* in_mul, const float* in_add,
                   int bf16, void* out, float* col_scratch, float* db, int cvalid, void* stream);
int virnet_conv_wgrad_f16(const void* xt, const void* yt, float* dw, float* scratch, int n, int h, int w, int cx, int cy, int cin, int cout,
                          int bf16, void* stream);
/* ... and, in the same reduction launch, the bias gradient from the column partials an emitting convolution left for yt's tensor
 * (virnet_t_emit.col, nblk from virnet_conv_emit_ok): db[c] += sum over blocks, c < cvalid (zero db first). */
int virnet_conv_wgrad_f16_db(const void* xt, const void* yt, float* dw, float* scratch, int n, int h, int w, int cx, int cy, int cin, int cout,
                             int bf16, const float* col, float* db, long nblk, int cvalid, void* stream);
/* The weight gradients of the two stride-2 layers on the same kernel (backward of DownBlock.downsampler networks/AttResUNet.py:67 and
 * UpBlock.upsampler :80).  The HIGH-resolution operand [n][h][w][c] (c % 32 == 0, w even) is re-laid by virnet_chsplit_s2 into a
 * column-phase T: one row per source row, [h+2][2*c/32 blocks][hi|lo][seg(w/2)][32 ch][8 px], block par*c/32 + k = the pixels
 * x = 2*ox + par of channel block k -- every tap of a stride-2 window is then an aligned 16-pixel run (or one shifted by a single T
 * pixel), and a step of the contraction (low-res row oy) reads the high-res rows 2oy-1 .. 2oy+1: two new ring rows per step.
 * The LOW-resolution operand [n][oh][ow][clo] is a plain virnet_chsplit T.
 *   mode 0: 3x3 stride-2 pad-1 conv, hi = the conv's input (cin real channels), lo = its output gradient (cout): dw[cout][cin][3][3]
 *   mode 1: 2x2 stride-2 transposed conv, hi = its output gradient (cout), lo = its input (cin):              dw[cin][cout][2][2]
 * dw is overwritten (fixed summation order: bitwise reproducible); scratch = virnet_conv_wgrad_f16_s2_scratch_bytes() bytes. */
size_t virnet_chsplit_s2_bytes(int n, int h, int w, int c);
size_t virnet_chsplit_s2_colsum_bytes(int n, int h, int w, int c);
int virnet_chsplit_s2(const float* x, int n, int h, int w, int c, int in_act, float in_slope, const float* in_mul, const float* in_add,
                      int bf16, void* out, float* col_scratch, float* db, int cvalid, void* stream);
size_t virnet_conv_wgrad_f16_s2_scratch_bytes(int n, int oh, int ow, int chi, int clo);
int virnet_conv_wgrad_f16_s2(const void* hi_t, const void* lo_t, float* dw, float* scratch, int n, int oh, int ow, int chi, int clo,
                             int cin, int cout, int mode, int bf16, void* stream);
/* What the three launchers above plan for a shape, without launching and without a device -- the same rule (one function) they launch
 * by, so the instantiation conv_wgrad_f16_kernel<nwv, bf16, kg, ..> and the split of the pixel range can be read off a call.
 *   mode 0: virnet_conv_wgrad_f16(_db), (h, w, cx, cy) as there
 *   mode 1 / 2: virnet_conv_wgrad_f16_s2 with its mode 0 / 1, (h, w) = its (oh, ow), (cx, cy) = its (chi, clo)
 * kg: 16-pixel k-steps per step (waves per channel block); nwv: output-channel blocks per workgroup; pairs: (output group, input block)
 * pairs; the nsteps = n * nxs * h steps (nxs column strips of 16 * kg pixels) are cut into `split` runs of `run` steps, run i = steps
 * [i * run, min((i + 1) * run, nsteps)) -- trailing runs can be empty; pairs * split workgroups; scratch = split * 9 * (32-padded output
 * channels) * (32-padded input channels) floats.  Returns 0, or nonzero for a shape the launcher rejects. */
typedef struct {
  int kg, nwv, pairs, split, run, nxs, nsteps;
} virnet_wgrad_f16_plan;
int virnet_conv_wgrad_f16_plan_query(int n, int h, int w, int cx, int cy, int mode, virnet_wgrad_f16_plan* out);
/* T emission (training step): a stride-1 3x3 NHWC convolution with a single-store epilogue (y_raw XOR y_act; residual and / or mask
 * allowed; no output SFT, no in_mul for the Winograd form) can write, besides its NHWC tensor, the channel-major T image of that
 * tensor -- exactly what a virnet_chsplit pass over it would produce, without reading it back (the 74 re-layout passes of a training
 * step were 13 % of it) -- and per-workgroup channel sums of it (the bias gradient of the conv whose output gradient this tensor is).
 *   t_out : virnet_chsplit_bytes(n, h, w, cout) bytes whose rows 0 / h+1 and pad segments are ALREADY zero (the kernel writes the image
 *           rows and, inside them, zeros for tile pixels beyond w; it never touches the pads) -- bf16 != 0: one bf16 plane
 *   act   : T holds lrelu(y, slope) instead of y (the staging transform of the NEXT conv, AttResUNet.py:55, whose weight gradient reads it)
 *   col   : NULL, or virnet_conv_emit_ok()'s nblk * cout floats: partial sums col[(cb * nblk + blk) * 32 + ch] of y over the pixels of
 *           workgroup-wave blk; virnet_colpart_reduce adds them into db (zero db first)
 * virnet_conv_emit_ok: 1 when `d` can run with emission in that form (0: virnet_conv_f16 / virnet_conv_bf16, 1: virnet_conv_wx4 with 16-row
 * tiles, 2: with 8-row tiles). */
typedef struct virnet_t_emit {
  void* t_out;
  float* col;
  int act;
  float slope;
  int bf16;
  int rows;    /* virnet_conv_wx4_emit: 0 / 16 = 16-row tiles (one workgroup per CU), 8 = 8-row tiles (two per CU: the image's stores
                  run beside the other workgroup's K loop); virnet_conv_emit_ok form 1 / 2 */
} virnet_t_emit;
int virnet_conv_emit_ok(const virnet_conv_desc* d, int form, int* nblk);
int virnet_conv_f16_emit(const virnet_conv_desc* d, const virnet_t_emit* te, int bf16_operands, void* stream);
int virnet_conv_wx4_emit(const virnet_conv_desc* d, const virnet_t_emit* te, void* stream);
int virnet_colpart_reduce(const float* col, float* db, long nblk, int ncb, int cvalid, void* stream);
/* Backward of the SFT pre-activation a = lrelu(x*mul + add, slope) with per-image [n][c] vectors (AttResUNet.py:54-58), given da = dL/da:
 * du = da * lrelu'(x*mul+add);  dx = du*mul (+ res, the skip gradient, may be NULL);  dmul[n][c] += sum_p du*x;  dadd[n][c] += sum_p du
 * (zero dmul / dadd first).  NHWC tensors of n images x hw pixels x c channels (c % 4 == 0). */
int virnet_sft_backward(const float* da, const float* x, const float* mul, const float* add, const float* res, float slope, float* dx,
                        float* dmul, float* dadd, int n, long hw, int c, void* stream);
/* The same backward (AttResUNet.py:54-58) with order-fixed sums: dx is bit for bit virnet_sft_backward's; dmul / dadd are WRITTEN (no
 * zero-initialisation, no atomics).  Each block of 1024 pixels stores its per-channel sums to partials[n][chunks][2][c] and a second
 * launch adds a channel's chunks in ascending order, so the result depends on (hw, c) only: it repeats from run to run and an image
 * gives the same bits alone and inside a batch.  partials: virnet_sft_backward_scratch_bytes(n, hw, c) bytes, 16-byte aligned (as dmul
 * and dadd), overlapping no input or output. */
size_t virnet_sft_backward_scratch_bytes(int n, long hw, int c);
int virnet_sft_backward_ordered(const float* da, const float* x, const float* mul, const float* add, const float* res, float slope,
                                float* dx, float* dmul, float* dadd, float* partials, int n, long hw, int c, void* stream);
/* db[c] += sum over pixels of dy[p][c], c < cvalid (NHWC rows of `c` stored channels, c % 4 == 0); zero db first */
int virnet_colsum(const float* dy, float* db, long npix, int c, int cvalid, void* stream);
/* z[n][2h][2w][c] = dy at even positions, 0 elsewhere: the stride-2 conv's dgrad is a stride-1 conv of z (AttResUNet.py:67) */
int virnet_zero_stuff2(const float* dy, float* z, int n, int h, int w, int c, void* stream);
/* out[n][h][w][(a*2+b)*c + k] = dy[n][2h+a][2w+b][k]: the transposed conv's dgrad / wgrad operand (AttResUNet.py:80) */
int virnet_space_to_depth2(const float* dy, float* out, int n, int h, int w, int c, void* stream);
/* Adjoint of virnet_pack_input for ONE map channel: dmap[n][h][w] (+)= sum over padded positions that read (y,x) of
 * drec[n][hp][wp][crec][chan] * (map_sqrt ? 0.5/sqrt(map[y][x]) : 1)   (reflect pad of util_net.py:20-25, sqrt of VIRNet.py:44) */
int virnet_pack_input_backward(const float* drec, int crec, int chan, const float* map, float* dmap, int n, int h, int w, int hp,
                               int wp, int map_sqrt, int accumulate, void* stream);

/* Image gradient of the network's entry convolutions (gradients with respect to the input image, frozen parameters): for the NCHW
 * image gradient dx[n][c][h][w], c < c0 <= 4,
 *   dx = (accumulate ? dx : 0)
 *      + sum_{a,b<sf} dres[n][c][sf*y+a][sf*x+b]                                        (dres: mu = tail + x_up, VIRNet.py:83; AttResUNet.py:173)
 *      + sum_{a,b<sf} sum_{P in refl^-1(sf*y+a, sf*x+b)} sum_{co,ky,kx} wa[co][c][ky][kx] * ga[n][P + (1-ky, 1-kx)][co]
 *        (ga: output gradient of a 3x3 pad-1 conv on records nearest-upsampled by sf and reflect-padded to hp x wp -- AttResUNet.head,
 *         AttResUNet.py:150-155, util_net.py:20-25; refl^-1 folds the bottom / right margins back onto their source rows / columns)
 *      + sum_{co,ky,kx} wb[co][c][ky][kx] * gb[n][y+1-ky][x+1-kx][co]                    (gb: DnCNN.conv1 at h x w, zero padding, DnCNN.py:38)
 * Each of dres / ga / gb may be NULL (term absent).  wa / wb are the forward OIHW weights [ca][cina][3][3] / [cb][cinb][3][3]; the image
 * is their first c0 input channels (the conditioning channels of a record keep their own route, virnet_pack_input_backward).  ga / gb
 * are NHWC fp32, 16-byte aligned, ca / cb multiples of 4.  fp32 FMA, no scratch. */
typedef struct virnet_image_grad_desc {
  const float* dres;   /* NCHW [n][c0][sf*h][sf*w] or NULL */
  const float* ga;     /* NHWC [n][hp][wp][ca] or NULL */
  const float* wa;     /* OIHW [ca][cina][3][3] */
  const float* gb;     /* NHWC [n][h][w][cb] or NULL */
  const float* wb;     /* OIHW [cb][cinb][3][3] */
  float* dx;           /* NCHW [n][c0][h][w] */
  int n, c0, h, w, sf;
  int hp, wp, ca, cina;
  int cb, cinb;
  int accumulate;
} virnet_image_grad_desc;
int virnet_image_grad(const virnet_image_grad_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * KNet pieces (networks/KNet.py) and the SFT generator (networks/AttResUNet.py:11-32).  Small, latency-bound kernels.
 * ---------------------------------------------------------------------------------------------- */

/* KernelNet.head: Conv2d(cin -> cout, k=9, s=4, p=4, bias=False) (KNet.py:45,53).  x NCHW [n][cin][h][w], w OIHW,
 * out NHWC [n][oh][ow][cout] with oh = (h-1)/4+1, ow = (w-1)/4+1; cout a multiple of 64. */
int virnet_conv_head_s4(const float* x, const float* w, float* out, int n, int cin, int h, int w_, int cout, void* stream);
/* Its weight gradient (SISR training step, train_SISR.py:207-224): dw[cout][cin][9][9] = sum_{n,oy,ox} dy[n][oy][ox][co] *
 * x[n][ci][4oy+ky-4][4ox+kx-4]; x NCHW, dy NHWC [n][oh][ow][cout]; dw is overwritten. */
int virnet_conv_head_s4_wgrad(const float* x, const float* dy, float* dw, int n, int cin, int h, int w_, int cout, void* stream);
/* Its input gradient (an image gradient through KNet, KNet.py:45,53): dx[n][ci][iy][ix] = sum over co, oy, ox with ky = iy+4-4oy and
 * kx = ix+4-4ox in [0, 9) of w[co][ci][ky][kx] * dy[n][oy][ox][co]; dy NHWC [n][oh][ow][cout] (16-byte aligned, cout % 4 == 0), dx NCHW
 * [n][cin][h][w_] is overwritten; any h, w_. */
int virnet_conv_head_s4_dgrad(const float* dy, const float* w, float* dx, int n, int cin, int h, int w_, int cout, void* stream);

/* Global average pool of a planar tensor [n][c][h][w] -> out[n][c], with the finishing op of its call site:
 *   VIRNET_GAP_MEAN      mean                                  (DnCNN.py:31,42)
 *   VIRNET_GAP_EXPCLAMP  exp(clamp(mean, lo, hi))              (VIRNet.py:81 on the pooled SNet output)
 *   VIRNET_GAP_KINFO     channels 0..c-2 exp(clamp(mean, lo, hi)), channel c-1 tanh(mean)   (KNet.py:50,56-59) */
enum { VIRNET_GAP_MEAN = 0, VIRNET_GAP_EXPCLAMP = 1, VIRNET_GAP_KINFO = 2 };
int virnet_gap_nchw(const float* x, float* out, int n, int c, int h, int w, int finish, float lo, float hi, void* stream);

/* CALayer gate (KNet.py:15-25): gate[n][c] = sigmoid(W2 lrelu0.2(W1 mean_hw(x[n]) + b1) + b2); x NHWC [n][h][w][c];
 * W1 [cr][c], W2 [c][cr] (the 1x1 conv weights); c <= 256 and a divisor of 256. */
int virnet_ca_gate(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                   int n, int h, int w, int c, int cr, void* stream);

/* RB_Layer tail (KNet.py:26,38): out = hcv * gate[n][c] + skip, all NHWC [n][h][w][c], c % 4 == 0. */
int virnet_scale_add(const float* hcv, const float* gate, const float* skip, float* out, int n, int hw, int c, void* stream);

/* CALayer + RB_Layer tail in one launch (KNet.py:15-26,38): out = hcv * sigmoid(W2 lrelu0.2(W1 mean_hw(hcv) + b1) + b2) + skip, for
 * maps of at most 16384 float4 items per image (h*w*c/4; KernelNet's 16x16x64 map has 4096): one workgroup holds an image in
 * registers.  Same arguments and limits as virnet_ca_gate / virnet_scale_add, which remain for larger maps. */
int virnet_ca_scale_add(const float* hcv, const float* w1, const float* b1, const float* w2, const float* b2, const float* skip,
                        float* out, int n, int h, int w, int c, int cr, void* stream);

/* KernelNet body as ONE persistent kernel (KNet.py:28-39,46-48,54: `nlayers` RB_Layers = conv3x3 + LeakyReLU(0.2) + conv3x3 + CALayer +
 * skip, each), one workgroup per image holding the h x w x 64 map on the CU (csrc/knet_body.hip): for maps of at most 16 x 16 pixels
 * (LR images up to 64 x 64 behind the stride-4 head).  x, y: NHWC [n][h][w][64] fp32 (y may alias x).  Per layer: w1pack / w2pack =
 * virnet_pack_f16_weight images of the two 64->64 convs (cin_pad = n_pad = 64), b1 / b2 their biases (NULL = none), caw1 [cr][64], cab1
 * [cr], caw2 [64][cr], cab2 [64] the CALayer's 1x1 convs.  Same split-fp16 arithmetic per product as virnet_conv_f16; the channel means
 * are summed in a fixed order (bitwise reproducible).  Larger maps: virnet_conv_f16 + virnet_ca_scale_add per layer. */
typedef struct virnet_knet_layer {
  const float *w1pack, *b1, *w2pack, *b2;
  const float *caw1, *cab1, *caw2, *cab2;
} virnet_knet_layer;
int virnet_knet_body(const float* x, float* y, const virnet_knet_layer* layers, int nlayers, int n, int h, int w, int c, int cr, void* stream);

/* AttLayer weights (AttResUNet.py:18-25), all 1x1 convs stored [cout][cin]. */
typedef struct virnet_sft_weights {
  const float *w1, *b1;   /* [nf1][e]   */
  const float *w2, *b2;   /* [nf2][nf1] */
  const float *wm, *bm;   /* [nf][nf2]  mul_conv (sigmoid) */
  const float *wa, *ba;   /* [nf][nf2]  add_conv */
  int e, nf1, nf2, nf;
} virnet_sft_weights;

/* Spatially constant conditioning: mul[n][nf], add[n][nf] from vec[n][e] (AttLayer.forward, AttResUNet.py:27-32). */
int virnet_sft_vec(const float* vec, const virnet_sft_weights* wt, float* mul, float* add, int n, void* stream);
/* The same for `nlayers` (1..16) AttLayers on ONE vector in one launch (every AttResBlock.sft1 / sft2 of the down path, AttResUNet.py:50,57,
 * depends on nothing but the conditioning vector): wts[l] -> muls[l][n][nf_l], adds[l][n][nf_l]; all layers take the same `e`.  (ABI 3) */
int virnet_sft_vec_multi(const float* vec, const virnet_sft_weights* wts, int nlayers, float* const* muls, float* const* adds, int n, void* stream);

/* Per-pixel conditioning: act = lrelu0.2(raw * mul(e) + add(e)) (AttResUNet.py:54-58) where e = channels
 * [chan0, chan0+wt->e) of the full-resolution 16-channel records rec[n][hp][wp][16] sampled at (y*step, x*step)
 * -- the nearest resize of AttResUNet.py:168.  raw/act NHWC [n][h][w][nf], hp = h*step, wp = w*step. */
int virnet_sft_apply(const float* raw, const float* rec, const virnet_sft_weights* wt, float* act, int n, int h, int w,
                     int step, int chan0, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation metrics on uint8 images (csrc/metrics.hip): what the reference's scripts compute on the host after every forward.  Every
 * operation that decides a rounding is fp64 or integer; results are bitwise reproducible and independent of the batch size.
 * ---------------------------------------------------------------------------------------------- */
/* skimage's img_as_ubyte as the reference's scripts apply it to a restored image (scripts/denoising_virnet_syn.py:138 after the clip):
 * out[i] = rint(double(clamp(x[i], 0, 1)) * 255.0), round half to even; NaN gives 0 (undefined on the host).  x fp32, out uint8, n values. */
int virnet_quantize_u8(const float* x, uint8_t* out, size_t n, void* stream);
/* MATLAB-style luma of utils/util_image.py:129-153 (only_y=True) on uint8: rgb NCHW [n][3][h][w] -> y [n][1][h][w] =
 * rint(fma(b, c2, fma(g, c1, r*c0)) + 16.0) in fp64, c = {65.481, 128.553, 24.966} / 255.0.  The order is part of the contract: 194 of the
 * 2^24 RGB triples have an exact value ending in .5 and round by it. */
int virnet_rgb2y_u8(const uint8_t* rgb, uint8_t* y, int n, int h, int w, void* stream);
/* PSNR and SSIM of utils/util_image.py:17-89 for n image pairs a, b: NCHW [n][c][h][w], c = 1 or 3, each uint8 or (x_f32 != 0) fp32 in
 * [0,1] that is quantised as by virnet_quantize_u8 while it is read.  ycbcr != 0 (c = 3): both are converted as by virnet_rgb2y_u8 first
 * and there is one metric channel, else c.  `border` pixels are cropped on every side.  Per image:
 *   sse[i]   = sum over the cropped region and metric channels of (a - b)^2, exact;   count[i] = its number of elements
 *              (PSNR = 20 log10(255 / sqrt(sse / count)) is left to the caller: the host's own double expression)
 *   ssim[i]  = mean over metric channels of the mean SSIM map (11x11 Gaussian window, valid region; C1 = (0.01*255)^2, C2 = (0.03*255)^2,
 *              sigma^2 = E[a^2] - mu^2); NaN when with_ssim == 0
 * win11: HOST pointer to the 11 normalised 1-D window weights (cv2.getGaussianKernel(11, 1.5), utils/util_image.py:23) in fp64; the
 * filter runs separably.  workspace: virnet_psnr_ssim_workspace_bytes() bytes, 8-byte aligned, need not be zeroed (per-tile partial sums,
 * added in a fixed order by a second launch).  h, w >= 11 + 2*border when with_ssim, >= 1 + 2*border otherwise.  sse / count int64 [n],
 * ssim fp64 [n], all device pointers. */
/* ycbcr = 2 (float32 inputs only): the Y channel of the FLOAT RGB image, formed in fp32 and quantised afterwards, as the training
 * scripts' test stage does (util_image.py:91-116 batch_PSNR / batch_SSIM with ycbcr=True -> rgb2ycbcrTorch :155-176):
 *   t_c = x_c * 255f;  k_c = fp32(coef_c) / 255f;  y = clamp((((t_r*k_r + t_g*k_g) + t_b*k_b) + 16f) / 255f, 0, 1)
 * every operation rounded to fp32 on its own; then as one-channel images.  ycbcr = 0 / 1 are unchanged.  Any other value is refused
 * (before this mode existed every non-zero value meant 1; a caller that passed another non-zero value must now pass 1). */
size_t virnet_psnr_ssim_workspace_bytes(int n, int c, int h, int w, int border, int ycbcr);
int virnet_psnr_ssim(const void* a, int a_f32, const void* b, int b_f32, int n, int c, int h, int w, int border, int ycbcr, int with_ssim,
                     const double* win11, void* workspace, int64_t* sse, int64_t* count, double* ssim, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SISR degradation y = D_sf(k_n (*) x_n) and its adjoints (csrc/degrade.hip): the operator of the training likelihood
 * (loss/ELBO_simple.py:55-59 through utils/util_sisr.py:127-144) and of the synthetic evaluation input (utils/util_sisr.py:146-166).
 * x NCHW fp32 [n][c][h][w]; kernel fp32 [n][k][k], one per sample, shared by the channels, applied as a cross-correlation; k odd,
 * 1..25; sf 1..4; p = k/2 < min(h, w); n*c <= 65535; h, w <= 32768.  The output is ceil(h/sf) x ceil(w/sf).  All pointers are device
 * pointers to contiguous tensors.  fp32 vector arithmetic, no atomics: bitwise reproducible, and independent of the batch an image is in.
 * ---------------------------------------------------------------------------------------------- */
#define VIRNET_BORDER_REFLECT 0   /* d c b | a b c d: F.pad(mode="reflect"), the training operator (util_sisr.py:131) */
#define VIRNET_BORDER_SYMMETRIC 1 /* c b a | a b c:   scipy.ndimage's "reflect", the evaluation operator (util_sisr.py:158) */
/* y[n][c][i][j] = sum_{u,v} kernel[n][u][v] * x[n][c][m(i*sf+u-p, h)][m(j*sf+v-p, w)], m the border map; only the kept samples are
 * computed (util_sisr.py:127-144 with downsampler 'direct'; sf = 1 is the blur that the bicubic route resizes).  clip01 != 0 clamps the
 * stored value to [0, 1] (util_sisr.py:159). */
int virnet_degrade_forward(const float* x, const float* kernel, float* y, int n, int c, int h, int w, int k, int sf, int border, int clip01,
                           void* stream);
/* Adjoint w.r.t. the image: gx[n][c][a][b] = sum over (i,u,j,v) with m(i*sf+u-p) = a, m(j*sf+v-p) = b of kernel[n][u][v] * gy[n][c][i][j]
 * (what autograd derives from util_sisr.py:127-144); gy [n][c][ceil(h/sf)][ceil(w/sf)], gx [n][c][h][w], every element written. */
int virnet_degrade_grad_image(const float* gy, const float* kernel, float* gx, int n, int c, int h, int w, int k, int sf, int border,
                              void* stream);
/* Adjoint w.r.t. the kernel: gk[n][u][v] = sum_{c,i,j} gy[n][c][i][j] * x[n][c][m(i*sf+u-p)][m(j*sf+v-p)] (the kernel gradient of
 * ELBO_simple.py:55-59).  workspace: virnet_degrade_grad_kernel_workspace_bytes() bytes (0 = bad arguments), 4-byte aligned, need not be
 * zeroed: fp32 partial sums per 16 x 32 tile of gy, added per sample in tile order in fp64 by a second launch. */
size_t virnet_degrade_grad_kernel_workspace_bytes(int n, int c, int h, int w, int k, int sf);
int virnet_degrade_grad_kernel(const float* gy, const float* x, float* gk, void* workspace, int n, int c, int h, int w, int k, int sf, int border,
                               void* stream);
/* Banded resample along the middle axis of a contiguous [outer][n_in][inner] view: out[b][o][r] = sum_t wgt[o][t] * in[b][idx[o][t]][r],
 * accumulated in fp64.  idx int32 [n_out][taps] (entries outside 0..n_in-1 are skipped), wgt fp64 [n_out][taps], both on the device.
 * Either in is fp32 and out fp64 (in_f64 0, out_f64 1) or the reverse: two calls, rows then columns, are the antialiased cubic resize of
 * util_sisr.py:141-142 with an fp64 intermediate, and with the transposed tables its adjoint. */
int virnet_resample_axis(const void* in, int in_f64, void* out, int out_f64, const int32_t* idx, const double* wgt, int taps, long long outer,
                         int n_in, int n_out, long long inner, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Denoising objective and its variance prior (csrc/elbo.hip): loss/ELBO_simple.py:12-53 as train_denoising_syn.py:172-176 calls it, and
 * utils/util_denoising.py:53-63 as train_denoising_real.py:164 does.  mu, im_noisy, im_gt NCHW fp32 [n][c][h][w]; sigma_est [n][cs][h][w]
 * and beta0 [n][cb][h][w] with cs, cb each 1 or c (a single channel is broadcast); n*h*w < 2^31; h, w <= 32768.  All pointers are device
 * pointers to contiguous tensors, 4-byte aligned; when every image pointer is 16-byte aligned and h*w is a multiple of four the kernels
 * use 16-byte accesses.  alpha0 and psi = digamma(alpha0 - 1) are single floats in device memory.  No atomics: bitwise reproducible.
 * ---------------------------------------------------------------------------------------------- */
/* Bytes of the value entry's workspace (0 = bad sizes): one fp64 (lh, kl_gauss, kl_Igamma) partial per workgroup, at most 24 KB. */
size_t virnet_elbo_workspace_bytes(int n, int c, int h, int w);
/* out4 = {loss, lh, kl_gauss, kl_Igamma} of ELBO_simple.py:23-53 for one restorer output, with beta = sigma_est * alpha0, a = alpha0 - 1:
 *   lh        = mean_{n,c,h,w} 0.5 (log beta - psi + (a / beta) ((im_noisy - mu)^2 + eps2)) + 0.5 log(2 pi)
 *   kl_gauss  = 0.5 mean_{n,c,h,w} (mu - im_gt)^2 / eps2
 *   kl_Igamma = mean over [n][max(cs,cb)][h][w] of a (beta0 / beta - 1) + a (log beta - log beta0)      (0 when with_klig == 0)
 *   loss      = lh + kl_gauss + kl_Igamma (fp32, in that order)
 * Elements are evaluated in fp32 and added in fp64: per thread, wave, workgroup, then by a second one-workgroup launch in index order.
 * workspace: virnet_elbo_workspace_bytes() bytes, 8-byte aligned, need not be zeroed. */
int virnet_elbo_value(const float* mu, const float* sigma_est, const float* im_noisy, const float* im_gt, const float* beta0,
                      const float* alpha0, const float* psi, float eps2, int with_klig, void* workspace, float* out4, int n, int c, int cs,
                      int cb, int h, int w, void* stream);
/* Gradients of  *grad_out * (w_data * (lh + kl_gauss) + w_klig * kl_Igamma)  in closed form: dmu [n][c][h][w], dsigma [n][cs][h][w] (the
 * likelihood part summed over the channels a one-channel sigma_est is broadcast against); every element of both is written.  grad_out: one
 * float in device memory (the upstream gradient); w_data, w_klig: host weights (1, 1 for the objective itself; 1/L and 0 for the further
 * outputs of an L-fold deep supervision, which share the variance term). */
int virnet_elbo_grad(const float* mu, const float* sigma_est, const float* im_noisy, const float* im_gt, const float* beta0,
                     const float* alpha0, const float* grad_out, float eps2, double w_data, double w_klig, float* dmu, float* dsigma, int n,
                     int c, int cs, int cb, int h, int w, void* stream);
/* Variance prior of the real-noise training (util_denoising.py:53-63): out[n][c][y][x] = max(sum_{u,v} taps[u] taps[v] *
 * (im_noisy - im_gt)^2[n][c][r(y+u-p, h)][r(x+v-p, w)], floor), r the reflect map `d c b | a b c d`, p = k/2.  taps: k fp64 weights in
 * device memory (cv2.getGaussianKernel(k, 0.3 ((k-1)/2 - 1) + 0.8), util_denoising.py:24-40); k odd, 1..31, p < min(h, w);
 * n*c <= 65535.  The squared error is formed while the tile is staged and filtered separably (rows, then columns) in fp64. */
int virnet_noise_estimate(const float* im_noisy, const float* im_gt, const double* taps, float* out, int n, int c, int h, int w, int k,
                          float floor, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SISR objective around the degradation (csrc/elbo_sisr.hip): loss/ELBO_simple.py:55-138 as train_SISR.py:207-224 calls it, with the
 * kernel of utils/util_sisr.py:26-58.  Additive under ABI version 5.  All pointers are device pointers to contiguous tensors, 4-byte aligned
 * (fp64 buffers 8-byte); the image passes use 16-byte accesses when the plane size h*w is a multiple of four and the image pointers are
 * 16-byte aligned.  Scalars that the caller keeps on the device (kappa0, alpha0, psi, upstream gradients) are single floats.  Sums are
 * formed in fp64 in an order fixed by the shape, without atomics: bitwise reproducible.  Workspaces need not be zeroed.
 * ---------------------------------------------------------------------------------------------- */
/* KernelNet head (ELBO_simple.py:66-80,123-131; util_sisr.py:26-58).  kinfo_est, kinfo_gt [n][3]; gamma [n][2]: standard-Gamma draws of shape
 * kappa0 - 1; rho_eps [n]: standard-normal draws; k 1..25 (odd or even), sf 1..4.  Per sample, in fp64:
 *   v_i = kinfo_est_i kappa0 / gamma_i,  rho = clamp(kinfo_est_2 + sqrt(r2) rho_eps, -1, 1),  S = [[v1, d], [d, v2]], d = sqrt(v1) sqrt(v2) rho
 *   kernel = softmax over the k*k taps of -0.5 z^T S^-1 z,  z = (row, col) - centre,  centre = k/2 + (shift ? 0.5 (sf - k % 2) : 0)
 * A sample whose det S is exactly zero or not finite gets 1e-5 added to both diagonal entries (that sample only).
 * kernel: [n][k][k]; out4 = {kl_knet, kl_k0, kl_k1, kl_k2}: kl_k0/1 = mean_n of the inverse-Gamma KL of ELBO_simple.py:12-14 with
 * beta_q = kappa0 kinfo_est_i, beta_p = kappa0 kinfo_gt_i, shape kappa0 - 1; kl_k2 = penalty0 * 0.5 mean_n (rho_est - rho_gt)^2 / r2;
 * kl_knet = (kl_k0 + kl_k1 + kl_k2) / 3 * penalty1 in fp32.  workspace: virnet_sisr_head_workspace_bytes(n) bytes ([n][3] fp64 addends). */
size_t virnet_sisr_head_workspace_bytes(int n);
int virnet_sisr_head_forward(const float* kinfo_est, const float* kinfo_gt, const float* gamma, const float* rho_eps, const float* kappa0,
                             double r2, double penalty0, double penalty1, int k, int sf, int shift, void* workspace, float* kernel, float* out4,
                             int n, void* stream);
/* dkinfo [n][3] = gradient of  <grad_kernel, kernel> + *grad_knet * kl_knet : v1, v2 receive the diagonal of dS only (the reference detaches
 * them in d), rho both off-diagonal entries where -1 <= kinfo_est_2 + sqrt(r2) rho_eps <= 1.  grad_kernel [n][k][k]. */
int virnet_sisr_head_backward(const float* kinfo_est, const float* kinfo_gt, const float* gamma, const float* rho_eps, const float* kappa0,
                              const float* grad_kernel, const float* grad_knet, double r2, double penalty0, double penalty1, int k, int sf,
                              int shift, float* dkinfo, int n, void* stream);
/* HR pass (ELBO_simple.py:16,57,108): zz = mu + sqrt(eps2) z_eps, out1 = kl_rnet = 0.5 mean (mu - im_hr)^2 / eps2.  [n][c][h][w] tensors,
 * n*c*h*w < 2^31.  workspace: virnet_sisr_hr_workspace_bytes() bytes (one fp64 partial per workgroup, at most 8 KB). */
size_t virnet_sisr_hr_workspace_bytes(int n, int c, int h, int w);
int virnet_sisr_hr_value(const float* mu, const float* im_hr, const float* z_eps, double eps2, void* workspace, float* zz, float* out1, int n,
                         int c, int h, int w, void* stream);
/* dmu = *grad_rnet * (mu - im_hr) / (eps2 n c h w) + grad_zz. */
int virnet_sisr_hr_grad(const float* mu, const float* im_hr, const float* grad_zz, const float* grad_rnet, double eps2, float* dmu, int n, int c,
                        int h, int w, void* stream);
/* LR pass (ELBO_simple.py:12-14,55-59,110-112): y (the degraded zz) and im_lr [n][c][h][w]; sigma_est [n][cs][h][w] when fs != 0, [n] (one
 * value per sample, cs = 1) when fs == 0; sigma_prior likewise with cp, fp; cs, cp each 1 or c.  With beta = sigma_est alpha0,
 * beta0 = sigma_prior alpha0, a = alpha0 - 1, psi = digamma(a):
 *   out2[0] = lh      = mean_{n,c,h,w} (0.5 (log beta - psi) + 0.5 (a / beta) (im_lr - y)^2) + 0.5 log(2 pi)
 *   out2[1] = kl_snet = mean over the broadcast shape of sigma_est and sigma_prior of a (beta0 / beta - 1) + a (log beta - log beta0)
 *   stats [n][2] fp64: per sample, sum (im_lr - y)^2 and the sum of sigma_prior over the KL's elements (read by the gradient entry).
 * workspace: virnet_sisr_lr_workspace_bytes() bytes ([n][workgroups per sample <= 256][4] fp64). */
size_t virnet_sisr_lr_workspace_bytes(int n, int c, int h, int w);
int virnet_sisr_lr_value(const float* y, const float* im_lr, const float* sigma_est, const float* sigma_prior, const float* alpha0,
                         const float* psi, void* workspace, double* stats, float* out2, int n, int c, int h, int w, int cs, int fs, int cp, int fp,
                         void* stream);
/* Gradients of  *grad_lh * lh + *grad_snet * kl_snet : dy [n][c][h][w]; dsigma in sigma_est's shape, summed over what it was broadcast
 * across (a per-sample sigma_est in closed form from stats).  Every element of both is written. */
int virnet_sisr_lr_grad(const float* y, const float* im_lr, const float* sigma_est, const float* sigma_prior, const float* alpha0,
                        const double* stats, const float* grad_lh, const float* grad_snet, float* dy, float* dsigma, int n, int c, int h, int w,
                        int cs, int fs, int cp, int fp, void* stream);
/* *loss = *lh + *kl_rnet + *kl_snet + *kl_knet in fp32, in that order (ELBO_simple.py:133). */
int virnet_sisr_finish(const float* lh, const float* kl_rnet, const float* kl_snet, const float* kl_knet, float* loss, void* stream);

/* ------------------------------------------------------------------------------------------------
 * JPEG round trip (csrc/jpeg.hip): what utils/util_image.py:236-257 (cv2.imencode + cv2.imdecode, the last step of utils/util_sisr.py:146-177
 * and of datasets/SISRDatasets.py:107-112) does to an 8-bit RGB image -- baseline 4:2:0 with libjpeg's defaults, without the lossless
 * entropy coding, in 32-bit integers; virnet_amd/jpeg.py lists the steps and roundtrip_np there is the definition.  Additive under ABI
 * version 5.  src, dst NCHW [n][3][h][w], each uint8 or (x_is_f32 != 0) fp32: an fp32 source is quantised as by virnet_quantize_u8 while it
 * is read, an fp32 destination receives (float)v * (float)(1.0 / 255.0).  qf: int32 [n] in device memory, one quality per sample, 1..100
 * (larger counts as 100); qf[i] <= 0 leaves sample i uncompressed: src is copied to dst, bit for bit when both have one type.  tables: int32
 * [101][2][64] in device memory, entry q = quality q's (luma, chroma) divisors in natural order, entry 0 unused.  workspace:
 * virnet_jpeg_workspace_bytes() bytes (0 = bad sizes), need not be zeroed: per sample the decoded Y plane and the two decoded half-size
 * chroma planes as uint8, n (h w + 2 ceil(h/2) ceil(w/2)).  n 1..65535, h, w 1..32768.  Two launches on `stream`, no synchronisation, no
 * atomics: bitwise reproducible, and independent of the batch an image is in.  dst may be src.
 * ---------------------------------------------------------------------------------------------- */
size_t virnet_jpeg_workspace_bytes(int n, int h, int w);
int virnet_jpeg_roundtrip(const void* src, int src_is_f32, void* dst, int dst_is_f32, const int32_t* qf, const int32_t* tables, void* workspace,
                          int n, int h, int w, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient-norm clipping and the Adam step (csrc/optim.hip): the nn.utils.clip_grad_norm_ calls and the torch.optim.Adam.step() of
 * train_denoising_syn.py:175-184, train_denoising_real.py:172-177 and train_SISR.py:224-229.  Additive under ABI version 5.  A call takes a
 * LIST of `count` fp32 tensors as parallel host arrays: device pointers (4-byte aligned, contiguous tensors), numel (1 .. 2^31 - 1) and the
 * clip set of each tensor (0 .. nsets - 1, or -1 for none).  The list must be ordered by clip set, tensors in no set last.  It is cut into
 * chunks of VIRNET_OPTIM_CHUNK elements (a tensor owns ceil(numel / chunk) consecutive chunks; one workgroup per chunk) and travels by value
 * in the kernel arguments, VIRNET_OPTIM_TABLE tensors per launch: no host-to-device copy, no synchronisation.  A tensor whose pointers
 * are all 16-byte aligned is accessed 16 bytes at a time, any other 4 bytes at a time; both forms give the same bits.  No atomics: sums
 * are formed in fp64 in an order fixed by the list of sizes, bitwise reproducible.
 * ---------------------------------------------------------------------------------------------- */
#define VIRNET_OPTIM_CHUNK 4096
#define VIRNET_OPTIM_TABLE 64
/* The plan of a list (host only, no device work): first_chunk[i] = chunk ordinal of tensor i's first chunk, table[i] = which launch carries
 * tensor i, set_first[s] / set_chunks[s] = the contiguous range of chunk ordinals of clip set s (0, 0 for an empty set). */
int virnet_optim_plan(const long long* numel, const int* set, int count, int nsets, int* first_chunk, int* table, int* set_first,
                      int* set_chunks);
/* Bytes of virnet_optim_grad_norms' workspace (0 = bad sizes): one fp64 partial per chunk of the tensors that are in a clip set. */
size_t virnet_optim_workspace_bytes(const long long* numel, const int* set, int count);
/* torch.nn.utils.clip_grad_norm_(set, max_norm[s]) (train_denoising_syn.py:182-183, train_SISR.py:226-228) up to the scaling, for every clip
 * set at once: total_norm[s] = (float)sqrt(sum over the set's gradients of g^2, in fp64), coef[s] = min(max_norm[s] / (total_norm[s] +
 * 1e-6f), 1) in fp32; a NaN norm gives a NaN coefficient (error_if_nonfinite=False).  max_norm: host array [nsets]; total_norm, coef:
 * device [nsets]; workspace: virnet_optim_workspace_bytes() bytes, 8-byte aligned, need not be zeroed.  Tensors in no set are ignored. */
int virnet_optim_grad_norms(void* const* g, const long long* numel, const int* set, int count, const float* max_norm, int nsets,
                            void* workspace, float* total_norm, float* coef, void* stream);
/* The clip's scaling and torch.optim.Adam.step() (train_denoising_syn.py:184, train_SISR.py:229; torch's single-tensor path) in one pass
 * over (p, g, m, v), with g' = g * coef[set] (g for a tensor in no set):
 *   g' = fma(weight_decay, p, g')  (weight_decay != 0);  m = fma(g' - m, 1 - beta1, m);  v = fma((1 - beta2) g', g', v beta2);
 *   p = fma(-step_size, m / (sqrt(v) / bc2_sqrt + eps), p)
 * step_size[i] = lr / (1 - beta1^t_i) and bc2_sqrt[i] = sqrt(1 - beta2^t_i) are per-tensor host values (t_i: the tensor's step count, from
 * 1).  coef: device [nsets] as written by virnet_optim_grad_norms (not read when nsets == 0).  write_back != 0 also stores g' (before the
 * weight decay) to the gradients of the tensors in a set: what the reference's in-place clip leaves behind. */
int virnet_optim_adam_step(void* const* p, void* const* g, void* const* m, void* const* v, const long long* numel, const int* set,
                           const float* step_size, const float* bc2_sqrt, int count, int nsets, const float* coef, float one_minus_beta1,
                           float beta2, float one_minus_beta2, float eps, float weight_decay, int write_back, void* stream);
/* g = g * coef[set] in place for the tensors in a set: the last step of clip_grad_norm_ for a caller that keeps another optimizer. */
int virnet_optim_scale_grads(void* const* g, const long long* numel, const int* set, int count, int nsets, const float* coef, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Exponential moving average of the weights (csrc/ema.hip; host side virnet_amd/ema.py).  Additive under ABI version 5.  A call takes a
 * LIST of `count` pairs of fp32 tensors as parallel host arrays: two device pointers (4-byte aligned, contiguous, distinct) and numel
 * (1 .. 2^31 - 1) per pair.  As for the optimizer the list is cut into chunks of VIRNET_OPTIM_CHUNK elements (one workgroup per chunk) and
 * travels by value in the kernel arguments, VIRNET_OPTIM_TABLE pairs per launch: no host-to-device copy, no synchronisation, no workspace,
 * no atomics.  A pair whose two pointers are both 16-byte aligned is accessed 16 bytes at a time, any other 4 bytes at a time; both forms
 * give the same bits.  A NULL list, count < 0 or a bad numel / pointer returns non-zero with virnet_last_error() set; count == 0 is a
 * no-op that returns 0.
 * ---------------------------------------------------------------------------------------------- */
/* e = e + w * (p - e), per element as three fp32 operations each rounded on its own (d = p - e; t = w * d; e = e + t): p == e leaves e
 * bitwise unchanged (a -0 aside, which becomes +0).  w: 0 .. 1, the host's 1 - decay rounded once to fp32.  p is read only. */
int virnet_ema_update(void* const* e, void* const* p, const long long* numel, int count, float w, void* stream);
/* Exchanges a[i] and b[i] element by element as 32-bit words: bit for bit, NaN payloads included. */
int virnet_ema_swap(void* const* a, void* const* b, const long long* numel, int count, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training batches synthesised on the device (csrc/datagen.hip) from a device-resident uint8 image pool: what the reference's dataset classes
 * do per sample on the host (datasets/DenoisingDatasets.py:74-99, 137-155, 217-253; datasets/SISRDatasets.py:66-104).  Additive under ABI
 * version 5.  The pool is HWC uint8 RGB, images back to back without padding; table: device int64 [images][3] = (byte offset, height,
 * width).  params: the device blob of a batch of n samples, 96 n bytes, 8-byte aligned, as sections of n values each -- eight 4-byte
 * sections (int32 image index, crop row, crop column, augmentation flag 0..7, niid 0/1, qf; fp32 std; one unused) followed by eight fp64
 * sections (sigma-map centre row, centre column, 2 scale^2, down, up; lambda_1^2, lambda_2^2, theta).  The kernels trust it: the caller
 * checks that every crop lies inside its image (virnet_amd/datagen.py does, before the upload).  One launch per call on `stream`, no
 * synchronisation, no atomics, no scratch: bitwise reproducible and independent of a sample's position in the batch.
 * ---------------------------------------------------------------------------------------------- */
#define VIRNET_DATAGEN_DENOISE 0
#define VIRNET_DATAGEN_PAIR 1
#define VIRNET_DATAGEN_HR 2
#define VIRNET_DATAGEN_MAX_PATCH 8192
#define VIRNET_DATAGEN_MAX_KERNEL 25
/* Crop p x p patches, convert, augment by the sample's flag as util_image.data_aug_np does (utils/util_image.py:391-434), write fp32 NCHW.
 *   DENOISE (SimulateTrain.__getitem__, DenoisingDatasets.py:217-253): out0 = im_noisy [n,3,p,p], out1 = im_gt [n,3,p,p], out2 =
 *     sigma_map_gt [n,1,p,p].  im_gt = u8 * fp32(1/255) (skimage's img_as_float32); sigma = the normalised Gaussian bump of
 *     generate_sigma_niid (:190-203) evaluated in fp64 and rounded to fp32, or fp32(down) where niid is 0 (generate_sigma_iid, :205-211);
 *     im_noisy = im_gt + fp32(noise * sigma), clamped to [0, 1] when clip != 0 (:236-240); sigma_map_gt = max(sigma^2, fp32(1e-10))
 *     (:245-247).  noise: fp32 [n,3,p,p] at SOURCE coordinates (before the augmentation, as in the reference), or NULL: drawn by
 *     virnet_datagen_normal's generator with element index e = (c p + i) p + j at source coordinates.
 *   PAIR (RealTrain / DataLMDB.__getitem__, :74-99, :137-155): out0 from pool_a, out1 from pool_b (same shapes, one table), u8 * fp32(1/255).
 *   HR (GeneralTrainFloder.__getitem__, SISRDatasets.py:66-76): out0 = u8 / 255 as a true fp32 division (util_image.imread,
 *     utils/util_image.py:206). */
int virnet_datagen_patches(int mode, const void* pool_a, const void* pool_b, const long long* table, const void* params, int n, int p,
                           const float* noise, const long long* sample_ids, unsigned long long seed, int stream_id, int clip, float* out0,
                           float* out1, float* out2, void* stream);
/* Standard normals in place of the torch.randn calls of DenoisingDatasets.py:236 and SISRDatasets.py:105: out fp32 [n][per].  Philox4x32-10
 * with key = seed and counter (e >> 2, stream_id, sample id low word, high word), e = 0 .. per - 1 within a sample; the word pairs (w0, w1)
 * and (w2, w3) each give two normals by Box-Muller with u1 = ((w >> 8) + 1) 2^-24, u2 = (w >> 8) 2^-24, r = sqrt(-2 log u1), (r cos 2 pi u2,
 * r sin 2 pi u2); element e takes normal e & 3.  sample_ids: device int64 [n]. */
int virnet_datagen_normal(float* out, int n, long long per, const long long* sample_ids, unsigned long long seed, int stream_id, void* stream);
/* util_sisr.shifted_anisotropic_Gaussian (utils/util_sisr.py:60-93) per sample in fp64: kernel fp32 [n,1,k,k] (k odd, <= 25), kinfo fp32
 * [n,3] = (var_x, var_y, rho).  lam1_sq, lam2_sq, theta: device fp64 [n].  One workgroup per sample. */
int virnet_datagen_blur_kernels(const double* lam1_sq, const double* lam2_sq, const double* theta, int n, int k, int sf, int shift, float* kernel,
                                float* kinfo, void* stream);
/* MixUp of the real-noise training (MixUp_AUG.aug, datasets/data_tools.py:19-30, applied to every batch by train_denoising_real.py:160-164).
 * mix: the device description of one batch's mix, 8 n bytes, 4-byte aligned: int32 perm[n] (each 0 .. n-1; the reference draws a
 * permutation, repeats are harmless since samples are only read through it), then fp32 lam[n] in [0, 1].  The entries do NOT validate its
 * contents: virnet_amd/datagen.py (MixParams.validate) does on the host before the upload, as for the parameter blob above.
 *   out_a[i] = lam[i] * a[i] + (1 - lam[i]) * a[perm[i]], and the same for b, for two fp32 tensors of n samples of `per` elements each:
 * 1 - lam, both products and the sum are each rounded to fp32 on their own, as the reference's separate torch ops round them.  One launch;
 * 16-byte accesses when per is a multiple of four and a, b, out_a, out_b are 16-byte aligned, 4-byte accesses otherwise.  n 1..65535, per
 * 1..2^31-1.  The gather makes an in-place mix wrong: an output that overlaps an input, the mix or the other output is refused. */
int virnet_mixup(const float* a, const float* b, const void* mix, float* out_a, float* out_b, int n, long long per, void* stream);
/* The PAIR mode of virnet_datagen_patches followed by that mix, in one launch (train_denoising_real.py:160-164 with
 * datasets/data_tools.py:19-30): out0 = im_noisy from pool_a, out1 = im_gt from pool_b, both [n,3,p,p].  One workgroup per 32 x 32 output
 * tile of sample i stages the tile's source rectangle of sample i and that of the same output tile of sample perm[i] -- which has its own
 * image, crop origin and augmentation flag -- from both pools, converts the four to u8 * fp32(1/255) and mixes as virnet_mixup does.
 * Nothing is read outside either crop.  Outputs that overlap each other, params or mix, or that contain the start of a pool or of the
 * table (whose extents the entry cannot know), are refused. */
int virnet_datagen_pair_mix(const void* pool_a, const void* pool_b, const long long* table, const void* params, const void* mix, int n, int p,
                            float* out0, float* out1, void* stream);
/* The validation set of the denoising training, SimulateTest.__getitem__ (datasets/DenoisingDatasets.py:255-296), for n pool images of one
 * common shape h x w: indices device int32 [n] (rows of `table`, repeats allowed; the caller checks that every one names an h x w image).
 * noise: the ONE fp32 array [h_max][w_max][3] of the whole set (rng.standard_normal, drawn and uploaded once); it is read with the row
 * stride of w_max, not of w.  sigma: fp32 [VIRNET_SIMTEST_MAP][VIRNET_SIMTEST_MAP], the peaks map rescaled to [10/255, 75/255].  ys device
 * int32 [h], xs device int32 [w]: the source indices of cv2.resize(..., INTER_NEAREST_EXACT), floor((dst + 0.5) * 256 / size), each
 * 0 .. VIRNET_SIMTEST_MAP - 1, built by the host in fp64.  Per output element
 *   im_gt = u8 / 255 (a true fp32 division: util_image.imread, utils/util_image.py:206),  im_noisy = im_gt + fp32(noise[y][x][c] * sigma[ys[y]][xs[x]])
 * with the product and the sum each rounded on their own, as numpy rounds them; both outputs fp32 [n][3][h][w].  One launch, one thread
 * per pixel; no atomics, no scratch, no synchronisation.  n 1..65535, h <= h_max, w <= w_max, h w < 2^31 / 3. */
#define VIRNET_SIMTEST_MAP 256
int virnet_datagen_simulate_test(const void* pool, const long long* table, const int* indices, const float* noise, const float* sigma,
                                 const int* ys, const int* xs, int n, int h, int w, int h_max, int w_max, float* im_noisy, float* im_gt,
                                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * The step log of a training loop (csrc/trainlog.hip): the scalars the reference reads with .item() on every step
 * (train_denoising_syn.py:186-198) stay on the device until the loop prints.  Additive under ABI version 5.  The log is one device
 * buffer of virnet_trainlog_bytes(k, capacity) bytes, 8-byte aligned: fp64 sums[k], then fp32 ring[capacity][k].
 * ---------------------------------------------------------------------------------------------- */
#define VIRNET_TRAINLOG_MAX 16
#define VIRNET_TRAINLOG_MAX_CAPACITY 65536
/* Bytes of a log of k values per step (1 .. VIRNET_TRAINLOG_MAX) and `capacity` rows; 0 with the error set when refused. */
size_t virnet_trainlog_bytes(int k, int capacity);
/* One step: src[s] (host array of nsrc device pointers, 4-byte aligned) holds count[s] consecutive fp32 values, k in all, in order.  The
 * pointers travel by value in the kernel arguments.  ring[slot][t] = x_t and sums[t] += (double)x_t / (double)num_iter, one thread per
 * value, no atomics: pushes of one stream run in step order, so a sum is bit for bit the double that `acc += x.item() / num_iter` builds
 * step by step on the host.  One launch, no synchronisation.  A source inside the log is refused. */
int virnet_trainlog_push(const void* const* src, const int* count, int nsrc, void* log, int k, int capacity, int slot, int num_iter, void* stream);
/* sums[t] = 0 on `stream` (the ring is left alone). */
int virnet_trainlog_reset(void* log, int k, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 8-way flip / rotation self-ensemble of the real-noise evaluation (csrc/ensemble.hip): the `--flip` loops of
 * scripts/denoising_virnet_real_sidd.py:113-154 and dnd_submission_py/pytorch_wrapper.py:15-47 without their host round trips; the
 * definitions are expand_np / reduce_np of virnet_amd/ensemble.py.  Additive under ABI version 5.  Orientation m of an image is
 * util_image.data_aug_np(image, m) (utils/util_image.py:391-436): m / 2 quarter turns counter-clockwise, then an up-down flip for odd m.
 * Modes 0, 1, 4, 5 keep h x w and modes 2, 3, 6, 7 give w x h, so the orientations of b sources live in two fp32 NCHW groups,
 * even [4b][c][h][w] and odd [4b][c][w][h], image index b * 4 + (position of m in (0,1,4,5) or (2,3,6,7)); for h == w the two may be the
 * halves of one [8b][c][h][h] tensor.  c 1 or 3, b 1..65535, h, w 1..2^20; modes 8, or 1 for the scripts' `--flip False` (orientation 0
 * only: even is [b][c][h][w], odd is not touched and may be NULL).  One launch per call on `stream`, 256-thread workgroups over
 * (32 x 32 tile, image), no synchronisation, no atomics, no scratch: bitwise reproducible and independent of an image's place in the batch.
 * ---------------------------------------------------------------------------------------------- */
/* src [b][h][w][c] (HWC, as the .mat files hold the blocks), uint8 or (src_is_f32 != 0) fp32 -> every orientation as fp32 NCHW.  uint8
 * becomes the correctly rounded quotient u / 255 (skimage's img_as_float in fp64, then .type(torch.float32):
 * denoising_virnet_real_sidd.py:123-125); fp32 (DND, pytorch_wrapper.py:22-24) passes through bit for bit. */
int virnet_ensemble_expand(const void* src, int src_is_f32, float* even, float* odd, int b, int h, int w, int c, int modes, void* stream);
/* The inverse on the restored orientations: each is turned back (util_image.inverse_data_aug_np, utils/util_image.py:438-466) and the eight
 * are averaged per pixel in fp32 -- pairwise == 0: acc = +0; acc += inv_m for m = 0..7; acc / 8 (denoising_virnet_real_sidd.py:121-136);
 * pairwise != 0: +0 + (((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7))), / 8, numpy's mean over a contiguous axis of eight
 * (pytorch_wrapper.py:33) -- then clipped to [0, 1].  dst: fp32 (dst_is_f32 != 0; np.clip: -0 and NaN pass) or uint8 as by
 * virnet_quantize_u8 (skimage's img_as_ubyte, denoising_virnet_real_sidd.py:150); [b][h][w][c] (chw == 0) or [b][c][h][w].  modes == 1:
 * the clip, quantisation and layout change of orientation 0 alone (:138-150, pytorch_wrapper.py:35-45). */
int virnet_ensemble_reduce(const float* even, const float* odd, void* dst, int dst_is_f32, int pairwise, int chw, int b, int h, int w, int c,
                           int modes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LPIPS v0.1 with the AlexNet backbone (csrc/lpips.hip): the third column of the SISR table, scripts/sisr_virnet_syn.py:158-161 (with
 * util_image.normalize_lpips, utils/util_image.py:118-126), from caller-supplied weights; the definition is distance_torch of
 * virnet_amd/lpips.py.  Additive under ABI version 5.  Images are [n][3][h][w], uint8 or (flag != 0) fp32 in [0,1], quantised as by
 * virnet_quantize_u8 while they are read; h, w >= 31; no tensor of the call may reach 2^31 elements.  Nine launches per virnet_lpips call
 * on `stream` (stem, 2 pools, 4 convolutions, score, finish), no synchronisation, no atomics, no allocation: all scratch lies in the
 * 256-byte aligned `workspace` of virnet_lpips_workspace_bytes.  Bitwise reproducible, independent of a pair's place in the batch and
 * symmetric in (a, b); identical images give exactly 0.
 * ---------------------------------------------------------------------------------------------- */
typedef struct virnet_lpips_weights {
  const float* conv_w[5]; /* device fp32, 16-byte aligned: conv1 [363][64] with k = (c * 11 + ky) * 11 + kx; conv2..5 [KS * KS * cin][cout]
                           * with k = (ky * KS + kx) * cin + c (5 x 5 x 64 -> 192, 3 x 3 x 192 -> 384, 3 x 3 x 384 -> 256, 3 x 3 x 256 -> 256) */
  const float* conv_b[5]; /* device fp32 [cout] */
  const float* lin[5];    /* device fp32 [64], [192], [384], [256], [256]: the 1 x 1 "lin" weights */
  float shift[3], scale[3]; /* the scaling layer: x -> (x - shift) / scale per channel, applied before conv1's zero padding */
} virnet_lpips_weights;
/* Bytes of workspace for a feature stack over `images` images of h x w and `pairs` distances (virnet_lpips: images = 2 n, pairs = n;
 * virnet_lpips_features: images = n, pairs = 0); 0 with the error set when the arguments are refused. */
size_t virnet_lpips_workspace_bytes(int images, int pairs, int h, int w);
/* out[i] = LPIPS(a[i], b[i]), device fp64 [n], n 1..32767 (scripts/sisr_virnet_syn.py:158-161). */
int virnet_lpips(const void* a, int a_f32, const void* b, int b_f32, int n, int h, int w, const virnet_lpips_weights* wts, void* workspace,
                 double* out, void* stream);
/* The five ReLU taps of x as fp32 NCHW copies (the features scripts/sisr_virnet_syn.py:158-161 compares): out1 [n][64][h1][w1],
 * out2 [n][192][h2][w2], out3 [n][384][h3][w3], out4 and out5 [n][256][h3][w3]; h1 = (h - 7) / 4 + 1, h2 = (h1 - 3) / 2 + 1,
 * h3 = (h2 - 3) / 2 + 1.  Ten launches. */
int virnet_lpips_features(const void* x, int x_f32, int n, int h, int w, const virnet_lpips_weights* wts, void* workspace, float* out1,
                          float* out2, float* out3, float* out4, float* out5, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient buckets of data-parallel training (csrc/gradsync.hip): what DistributedDataParallel's reducer does around the all-reduce
 * (train_denoising_syn.py:71, train_denoising_real.py:70, train_SISR.py:95) -- gradients into a flat fp32 bucket, bucket slices back into
 * gradients.  Additive under ABI version 5.  A call takes a LIST of `count` fp32 tensors as parallel host arrays: device pointers (4-byte
 * aligned, contiguous tensors), numel (0 .. 2^31 - 1; an empty tensor is skipped) and the element offset of each tensor's slot in the
 * bucket; a slot must lie inside the bucket's bucket_numel elements (refused otherwise), offsets are otherwise arbitrary and slots are
 * the caller's to keep disjoint.  The list travels by value in the kernel arguments, VIRNET_GRADSYNC_TABLE tensors per launch, cut into
 * chunks of VIRNET_GRADSYNC_CHUNK elements laid over the destination's 16-byte grid: whole quads are stored 16 bytes at a time (and
 * loaded so when the source shares the destination's 16-byte phase), the quads cut by a slot's ends 4 bytes at a time; every element
 * goes through one fp32 multiply either way.  No atomics, no workspace, no synchronisation: both calls can be captured.
 * ---------------------------------------------------------------------------------------------- */
#define VIRNET_GRADSYNC_CHUNK 4096
#define VIRNET_GRADSYNC_TABLE 128
/* Launches a call with these sizes makes: ceil(non-empty tensors / VIRNET_GRADSYNC_TABLE). */
int virnet_gradsync_launches(const long long* numel, int count);
/* bucket[offset[i] + k] = src[i][k] * scale -- the bits of bucket[off:off+n].copy_(g).mul_(scale).  src[i] == NULL writes +0 to the
 * slot (a parameter that produced no gradient this step).  Bucket words outside every slot are not touched. */
int virnet_gradsync_pack(void* const* src, const long long* numel, const long long* offset, int count, float* bucket, long long bucket_numel,
                         float scale, void* stream);
/* dst[i][k] = bucket[offset[i] + k] * f -- the bits of bucket[off:off+n].clone().mul_(f); f = *scale_dev (one device float, read by the
 * kernel: the fused backward's un-scale never visits the host) when scale_dev != NULL, else `scale`.  dst[i] may be a fresh tensor or an
 * existing gradient; it must not overlap the bucket. */
int virnet_gradsync_unpack(const float* bucket, long long bucket_numel, const long long* offset, const long long* numel, void* const* dst,
                           int count, float scale, const float* scale_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Tiled restoration of a whole photograph (csrc/restore.hip): the two ends of utils/tiling.forward_tiled's loop on the device; the
 * definitions are gather_np / blend_np of virnet_amd/restore.py.  Additive under ABI version 5.  Only these two calls see the whole
 * image; the forward between them sees one batch of tiles.  1..4 channels.  No atomics, no workspace, no synchronisation: both calls
 * can be captured, are bitwise reproducible and do not depend on how the boxes are cut into calls.
 * ---------------------------------------------------------------------------------------------- */
#define VIRNET_TILE_BOXES 64
#define VIRNET_TILE_SLOTS 3
/* n (1..VIRNET_TILE_BOXES) boxes of th x tw pixels of the device image src -- uint8 or (src_is_f32 != 0) fp32, [h][w][c] or
 * (src_chw != 0) [c][h][w], h * w * c < 2^31 -- as one fp32 NCHW batch dst [n][c][th][tw].  boxes: HOST array of n (y, x) pairs, each box
 * inside the image (refused otherwise); it travels in the kernel arguments.  uint8 becomes the correctly rounded quotient u / 255
 * (np.float32(u / 255.0)), fp32 passes through bit for bit. */
int virnet_tile_gather(const void* src, int src_is_f32, int src_chw, int h, int w, int c, const int* boxes, int n, int th, int tw, float* dst,
                       void* stream);
/* The restored stack tiles [ny * nx][c][th][tw] (tile iy * nx + ix starts at output row min(iy * step_y, last_y), last_y = ho - th, and
 * column min(ix * step_x, last_x), last_x = wo - tw; fewer than 2^31 elements) -> one image dst of ho x wo pixels, [ho][wo][c] or
 * (chw != 0) [c][ho][wo], uint8 as by virnet_quantize_u8 or (dst_is_f32 != 0) fp32, clipped to [0, 1] like np.clip when clip != 0 (uint8
 * always is).  The tap tables are DEVICE arrays, 16-byte aligned: row_idx / row_w [VIRNET_TILE_SLOTS][row_pitch] give for output row q the
 * tile rows that cover it in ascending order (-1 = unused slot) and their fp32 weights, col_idx / col_w [VIRNET_TILE_SLOTS][col_pitch] the
 * same for the columns; pitches are multiples of four and at least ho / wo.  crop != 0: the value of tile (row_idx[0][qy], col_idx[0][qx])
 * is copied.  Otherwise acc = +0 and, over the used row slots and inside them the used column slots in ascending order,
 * acc = fl(acc + fl(fl(wy * wx) * v)); unused slots are skipped.  A slot that points outside the stack is skipped too. */
int virnet_tile_blend(const float* tiles, const int* row_idx, const float* row_w, const int* col_idx, const float* col_w, int row_pitch,
                      int col_pitch, int ny, int nx, int c, int th, int tw, int step_y, int last_y, int step_x, int last_x, int ho, int wo,
                      void* dst, int dst_is_f32, int chw, int clip, int crop, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training previews (csrc/preview.hip): what train_denoising_syn.py:199-212, train_denoising_real.py:192-205 and train_SISR.py:244-264
 * hand to their summary writer; the definitions are grid_np / kernel_np of virnet_amd/preview.py.  Additive under ABI version 5.  No
 * atomics, no synchronisation, the only workspace is the caller's: both calls can be captured and are bitwise reproducible.
 * ---------------------------------------------------------------------------------------------- */
/* bytes of virnet_preview_grid's workspace for a batch of b images: lo and the divisor per image */
size_t virnet_preview_grid_workspace_bytes(int b);
/* vutils.make_grid(x, nrow, padding, normalize=True, scale_each=True) followed by the summary writer's uint8 conversion, in two launches.
 * x: b images of c (1 or 3) planes of h x w, image i at x + i * batch_stride (elements; batch_stride >= c * h * w, so the first c channels
 * of a wider batch need no copy; b * batch_stride < 2^31).  out: uint8 [hg][wg][3], any alignment, hg * wg * 3 < 2^31.  b == 1: the bare
 * image, hg = h, wg = w.  Otherwise xmaps = min(nrow, b), ymaps = ceil(b / xmaps), hg = ymaps * (h + padding) + padding, wg = xmaps *
 * (w + padding) + padding, image i at row (i / xmaps) * (h + padding) + padding, column (i % xmaps) * (w + padding) + padding, every other
 * pixel 0; hg and wg are checked against this.  clamp != 0: every element is clipped to [lo, hi] as it is loaded (NaN passes); x itself
 * is not written.  Per image lo' and hi' are the minimum and maximum of its finite elements, d = float32(max(double(hi') - double(lo'),
 * 1e-5)), and a byte is trunc(clip(fl(fl(fl(v - lo') / d) * 255), 0, 255)) with a correctly rounded division; NaN and -inf give 0, +inf
 * 255, an image without a finite element is all 0.  c == 1: the plane goes to all three channels. */
int virnet_preview_grid(const float* x, long long batch_stride, int b, int c, int h, int w, int nrow, int padding, int clamp, float lo,
                        float hi, float* workspace, uint8_t* out, int hg, int wg, void* stream);
/* util_sisr.kinfo2sigma (util_sisr.py:26-58, 95-107): kinfo [n][3] = (variance x, variance y, rho) -> kernel [n][1][k][k], k <= 25, in
 * fp64 from the fp32 inputs: covariance [[v1, d], [d, v2]] with d = sqrt(v1) sqrt(v2) rho, its closed-form inverse, and a softmax of
 * -0.5 z' S^-1 z over the k * k positions z = (row, column) - centre, centre = k / 2 (+ 0.5 * (sf - k % 2) when shift != 0).  A sample
 * whose determinant is exactly zero or not finite gets 1e-5 on both diagonal entries, that sample only.  One workgroup per sample. */
int virnet_kernel_from_kinfo(const float* kinfo, int n, int k, int sf, int shift, float* kernel, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIRNET_HIP_H */
