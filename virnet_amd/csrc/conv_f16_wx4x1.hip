// conv_f16_wx4x1.hip -- the stride-1 3x3 convolution in Winograd F(4,3) form along x with ONE fp16 product per position product
// (gfx950): the reduced-precision inference form, VIRNET_CONV_FORM=wx4x1.
//
// Call sites as conv_f16_wx4.hip (AttResBlock.conv1/conv2, networks/AttResUNet.py:43,46,55,58; DnCNN mid convs, networks/DnCNN.py:25-28),
// forward only.  Arithmetic: the weights are the hi pieces of the virnet_pack_wx4_weight image, fp16(U * 2^e); V = B^T x is formed in
// fp32 while staging exactly as conv_wx4_kernel does and rounded once to fp16; one v_mfma_f32_32x32x16_f16 per (position, row tap,
// 16-channel chunk) with fp32 accumulation: 18 MFMAs per 4 output pixels against 54 in the three-product form and 36 in conv_bf16 -- with
// 11-bit instead of 8-bit significands.  Inverse scale, A^T, bias, mask, residual, output SFT and activation stay in fp32.
//
// The kernel IS conv_wx4_kernel (conv_f16_wx4.hip, included below with WX4_X1 = 1): same tile (16 x 32 pixels x 32*NREP channels, 8
// waves), same single-buffered V replaced on the fly, same DMA-streamed U, same epilogue.  What the switch changes:
//   V: hi planes only, 27 KB instead of 54;  U stage: 6*NREP 1-KB pieces instead of 12*NREP (the lo pieces of the image are skipped);
//   staging: no lo split (pSub / pLo / hSub / hLo), one ds_write_b64 per position instead of a write2;
//   a stage: 3*NREP MFMAs, placed by tools/gen_wx4_sched.py --products 1 (conv_f16_wx4x1_sched.inc).
// The staging work of a stage (pixel loads, pre-activation, B^T, the fp16 round, LDS stores) was sized to hide behind 9*NREP MFMAs; behind
// 3*NREP it does not, so this kernel is bound by its staging VALU work, not by the matrix pipe (profiles/wx4x1_device.md).  The
// exchange buffer of the epilogue (112 KB) still holds the workgroup to one per CU.
// Host side: ONE tile form, so the plan (conv_plan.h: plan_wx4x1) is the slab grouping alone.
#define WX4_X1 1
#include "conv_f16_wx4.hip"

int virnet::plan_wx4x1_desc(const virnet_conv_desc* d, int& n_cu, ConvPlan& p) {
  VIRNET_REQUIRE(d != nullptr, "virnet_conv_wx4x1: desc is NULL");
  VIRNET_REQUIRE(d->x && d->wpack, "virnet_conv_wx4x1: x / wpack is NULL");
  VIRNET_REQUIRE(d->ks == 3 && d->stride == 1 && d->epi == VIRNET_EPI_NHWC, "virnet_conv_wx4x1: only the stride-1 3x3 NHWC conv (ks=%d stride=%d epi=%d)",
                 d->ks, d->stride, d->epi);
  if (int rc = check_conv_desc(d, "virnet_conv_wx4x1", true)) return rc;
  static int dev_cu = 0;
  if (n_cu <= 0) {
    if (dev_cu == 0) {
      int dev = 0;
      if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&dev_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || dev_cu <= 0) dev_cu = 256;
    }
    n_cu = dev_cu;
  }
  const int nb = d->n_pad / 32;
  const ConvKnobs kn = read_conv_knobs(KNOBS_WX4, nb);
  VIRNET_REQUIRE(plan_wx4x1(ConvShape{d->n, d->h, d->w, nb}, kn, n_cu, p) == 0, "virnet_conv_wx4x1: more launches than a plan holds");
  return 0;
}

// one launch of the plan -> its template instantiation
static int launch_wx4x1_planned(const FArgs& kk, int nrep, int epi, int pre, hipStream_t st) {
#define VIRNET_WX4X1_EPI(N_, E_)                                                                                               \
  if (epi == E_) return pre == 2 ? launch_wx4x1<N_, E_, 2>(kk, st) : pre == 1 ? launch_wx4x1<N_, E_, 1>(kk, st) : launch_wx4x1<N_, E_, 0>(kk, st);
#define VIRNET_WX4X1_CASE(N_)                                                                            \
  if (nrep == N_) {                                                                                      \
    VIRNET_WX4X1_EPI(N_, 0) VIRNET_WX4X1_EPI(N_, 1) VIRNET_WX4X1_EPI(N_, 2) VIRNET_WX4X1_EPI(N_, 3) VIRNET_WX4X1_EPI(N_, 4)                \
  }
  VIRNET_WX4X1_CASE(3) VIRNET_WX4X1_CASE(2) VIRNET_WX4X1_CASE(1)
#undef VIRNET_WX4X1_CASE
#undef VIRNET_WX4X1_EPI
  return virnet::set_error("virnet_conv_wx4x1: no kernel for nrep=%d epi=%d", nrep, epi);
}

extern "C" int virnet_conv_wx4x1(const virnet_conv_desc* d, void* stream) {
  ConvPlan p;
  int n_cu = 0;
  if (int rc = virnet::plan_wx4x1_desc(d, n_cu, p)) return rc;
  FArgs k = fargs_from_desc(d);
  hipStream_t st = static_cast<hipStream_t>(stream);
  k.range_flag = virnet::range_flag_ptr();
  k.store_nt = virnet::store_nt_for((size_t)d->n * d->h * d->w * d->cout * 4);
  const int epi = epi_of(d), pre = pre_of(d);
  for (int i = 0; i < p.n; ++i) {
    FArgs kk = k;
    kk.slab_base = p.l[i].slab_base;
    kk.NP = p.l[i].groups * p.l[i].nrep * 32;
    if (int rc = launch_wx4x1_planned(kk, p.l[i].nrep, epi, pre, st)) return rc;
  }
  return 0;
}
