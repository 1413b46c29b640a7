// conv_exit.hip -- the few-output-channel 3x3 exit convolutions with planar (NCHW) store: AttResUNet.tail 96 -> 3 + crop + `+ x_in`
// (networks/AttResUNet.py:139,173), DnCNN.conv_last 64 -> 1|2 + exp(clamp(.)) (DnCNN.py:29,41; VIRNet.py:43), KernelNet.tail 64 -> 3
// (KNet.py:49).  gfx950, split-fp16 MFMA products as conv_f16.hip.
//
// Taps as GEMM ROWS.  With cout * 9 <= 32 the convolution is a POINTWISE GEMM to rows (c, tap) followed by a shift-add:
//     z[(c, dy, dx)][p] = sum_ci w[c][ci][dy][dx] * x[ci][p]            one 32-row MFMA block holds all 27 (or 9, 18) rows
//     out[c][y][x]      = bias[c] + sum_{dy,dx} z[(c, dy, dx)][y + dy - 1][x + dx - 1]
// conv_f16's planar form spends a 32-row block on 3 channels for EVERY tap (27 useful of 288 rows per pixel and chunk); here every MFMA row
// is a (channel, tap) pair: 9x fewer MFMAs, and -- the point -- no halo tile of the input in LDS at all: a pixel is the column of exactly
// one MFMA, so its B fragment (8 channels of a 16-channel chunk per lane) goes global -> registers -> split -> MFMA.  What remains is
// reading the input once: the kernel is HBM-bound (algorithmic bytes = N*H*W*Cin*4 in + 4 B per output value).
//
// Workgroup = 4 waves = one 8 x 32 output tile.  Its z is needed on the 10 x 34 halo = 340 pixels, walked as 11 blocks of 32 (flat
// index, 12 surplus columns masked); block b belongs to wave b % 4.  Per block: Cin/16 chunks x (2 x 16-byte buffer loads -- a lane
// outside the halo / the image reads zeros through an out-of-range offset -- exact hi/lo split, 3 MFMAs); two blocks per wave in flight;
// A fragments (2 KB per chunk) sit in LDS.  z goes to LDS RAW as [row][pixel] fp32; then thread = output pixel sums its 9 z values per
// channel times the row's inverse weight scale (a scalar), applies bias and the planar epilogue (VIRNET_NCHW_*) and stores 128-byte runs.
// Nothing is read from global memory between the first pixel request and the last store except the pixels: scales, biases and the
// residual's values are requested at the top (round 5, tools/exit_timeline.py: per-register scale loads inside the block loop and
// per-channel scale / bias / residual loads behind the previous channel's store were 16 + 3 dependent round trips per tile, 0.28 -> 0.22 ms).
#include "conv_f16_common.h"

namespace {
using namespace virnet;

constexpr int EX_TH = 8, EX_TW = 32;
constexpr int EX_HW = EX_TW + 2;                 // halo row length
constexpr int EX_HPX = (EX_TH + 2) * EX_HW;      // 340
constexpr int EX_BLK = (EX_HPX + 31) / 32;       // 11
constexpr int EX_ZS = EX_BLK * 32 + 4;           // z row stride (floats)

// The kernel's body is conv_exit_body.inc, included into the two kernels below (one text; the plain kernels compile to the instructions they
// had before the additive map existed -- compared function by function, profiles/tail_compose.md).
// ZADD (the composed tail, engine.rnet_forward): an additive partial map `zadd` -- NHWC fp32, 32 channels = the rows of z at their TRUE
// scale, on the same H x W -- is added to a pixel block's accumulators before z goes to LDS: z = A x + zadd.  Requested with the block's
// pixel loads through a buffer descriptor of its own (a halo pixel outside the image reads zeros: z of the zero padding stays zero);
// brought to the raw accumulator's scale exactly, by the reciprocal of the row's inverse scale (both powers of two).
template <int NCH>      // 16-channel chunks of the input (0: runtime count)
__global__ __launch_bounds__(256) void conv_exit_kernel(const FArgs a) {
  constexpr bool ZADD = false;
  [[maybe_unused]] const float* const zadd = nullptr;
#include "conv_exit_body.inc"
}

template <int NCH>
__global__ __launch_bounds__(256) void conv_exit_zadd_kernel(const FArgs a, const float* __restrict__ zadd) {
  static_assert(NCH != 0, "the additive map rides on the buffer loads of the fixed-count forms");
  constexpr bool ZADD = true;
#include "conv_exit_body.inc"
}

// rows (c, tap = dy*3 + dx) of the pointwise GEMM: per-row power-of-two scale (largest scaled magnitude in [8192, 16384)), split image
// [chunk][hi|lo][lane = row + 32*(k>>3)][k&7] preceded by the 32 inverse scales.  One block.
__global__ void pack_exit_kernel(const float* __restrict__ w, int cout, int cin, int cin_pad, float* __restrict__ inv_scale, char* __restrict__ img) {
  const int nrows = cout * 9;
  __shared__ int eb[32];
  if (threadIdx.x < 32) {
    const int row = threadIdx.x;
    float m = 0.f;
    if (row < nrows) {
      const int c = row / 9, t = row - c * 9;
      for (int k = 0; k < cin; ++k) m = fmaxf(m, fabsf(w[((size_t)c * cin + k) * 9 + t]));
    }
    int e = 0;
    if (m > 0.f) { frexpf(m, &e); e = 14 - e; }
    e = max(-100, min(100, e));
    eb[row] = e;
    inv_scale[row] = ldexpf(1.f, -e);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 32 * cin_pad; i += blockDim.x) {
    const int row = i / cin_pad, k = i - row * cin_pad;
    float v = 0.f;
    if (row < nrows && k < cin) {
      const int c = row / 9, t = row - c * 9;
      v = ldexpf(w[((size_t)c * cin + k) * 9 + t], eb[row]);
    }
    const int chunk = k >> 4, kk = k & 15;
    const size_t base = (size_t)chunk * 2048 + (size_t)(row + 32 * (kk >> 3)) * 16 + (kk & 7) * 2;
    const _Float16 hi = (_Float16)v;
    *reinterpret_cast<_Float16*>(img + base) = hi;
    *reinterpret_cast<_Float16*>(img + base + 1024) = (_Float16)(v - (float)hi);
  }
}

template <int NCH>
int launch_exit(FArgs k, hipStream_t st) {
  const int nch = k.Cin >> 4;
  const int lds = nch * 2048 + (k.cout * 9 + 1) * EX_ZS * 4;    // A fragments + the (channel, tap) rows of z + the dummy row
  static unsigned long long attr_done = 0;
  auto kern = conv_exit_kernel<NCH>;
  if (virnet::first_use_on_device(attr_done)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return virnet::set_error("hipFuncSetAttribute(conv_exit): %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)(8 * k.tiles_per_xcd)), dim3(256), lds, st, k);
  return virnet::check_launch("conv_exit launch");
}

template <int NCH>
int launch_exit_zadd(FArgs k, const float* zadd, hipStream_t st) {
  const int lds = NCH * 2048 + (k.cout * 9 + 1) * EX_ZS * 4;
  static unsigned long long attr_done = 0;
  auto kern = conv_exit_zadd_kernel<NCH>;
  if (virnet::first_use_on_device(attr_done)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return virnet::set_error("hipFuncSetAttribute(conv_exit, z_add): %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)(8 * k.tiles_per_xcd)), dim3(256), lds, st, k, zadd);
  return virnet::check_launch("conv_exit(z_add) launch");
}

#ifdef VIRNET_F16_TIMING
long long* g_xlog = nullptr;
#endif
}  // namespace

#ifdef VIRNET_F16_TIMING
extern "C" void virnet_debug_exit_timing_buffer(void* p) { g_xlog = static_cast<long long*>(p); }   // tools/exit_timeline.py
#endif

extern "C" size_t virnet_exit_weight_floats(int cin_pad) { return 32 + (size_t)cin_pad * 32; }      // 32 scales + cin_pad/16 x 2 KB

extern "C" int virnet_pack_exit_weight(const float* w, int cout, int cin, int cin_pad, float* packed, void* stream) {
  VIRNET_REQUIRE(w && packed, "virnet_pack_exit_weight: NULL pointer");
  VIRNET_REQUIRE(cout >= 1 && cout * 9 <= 32, "virnet_pack_exit_weight: cout=%d: the (channel, tap) rows must fit one 32-row block (cout <= 3)", cout);
  VIRNET_REQUIRE(cin >= 1 && cin_pad % 16 == 0 && cin_pad >= cin, "virnet_pack_exit_weight: cin_pad=%d does not cover cin=%d", cin_pad, cin);
  hipLaunchKernelGGL(pack_exit_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), w, cout, cin, cin_pad, packed,
                     reinterpret_cast<char*>(packed + 32));
  return virnet::check_launch("pack_exit launch");
}

static int conv_exit_host(const virnet_conv_desc* d, const float* z_add, bool with_z, void* stream) {
  VIRNET_REQUIRE(d != nullptr, "virnet_conv_exit: desc is NULL");
  VIRNET_REQUIRE(d->x && d->wpack && d->y_raw, "virnet_conv_exit: x / wpack / y_raw is NULL");
  VIRNET_REQUIRE(d->ks == 3 && d->stride == 1 && d->epi == VIRNET_EPI_NCHW, "virnet_conv_exit: only the stride-1 3x3 conv with planar store (ks=%d stride=%d epi=%d)",
                 d->ks, d->stride, d->epi);
  VIRNET_REQUIRE(d->n > 0 && d->h > 0 && d->w > 0, "virnet_conv_exit: empty input n=%d h=%d w=%d", d->n, d->h, d->w);
  VIRNET_REQUIRE(d->cout >= 1 && d->cout * 9 <= 32, "virnet_conv_exit: cout=%d (the (channel, tap) rows must fit one 32-row block: cout <= 3)", d->cout);
  VIRNET_REQUIRE(d->cin_pad >= 16 && d->cin_pad % 16 == 0 && d->cin_pad <= 1024, "virnet_conv_exit: cin_pad=%d", d->cin_pad);
  VIRNET_REQUIRE(d->crop_h >= 1 && d->crop_h <= d->h && d->crop_w >= 1 && d->crop_w <= d->w, "virnet_conv_exit: crop %d x %d outside %d x %d", d->crop_h, d->crop_w, d->h, d->w);
  VIRNET_REQUIRE(d->nchw_op != VIRNET_NCHW_ADD || d->res, "virnet_conv_exit: VIRNET_NCHW_ADD without res");
  VIRNET_REQUIRE(d->res_sf >= 1 && d->crop_h % d->res_sf == 0 && d->crop_w % d->res_sf == 0, "virnet_conv_exit: res_sf=%d does not divide the crop", d->res_sf);
  VIRNET_REQUIRE(!d->mask && !d->mul && !d->in_mul && !d->y_act, "virnet_conv_exit: plain planar epilogue only");
  VIRNET_REQUIRE((long)d->h * d->w * d->cin_pad * 4 < (1L << 31), "virnet_conv_exit: one image's input (%d x %d x %d fp32) must stay below 2 GB (32-bit buffer offsets)", d->h, d->w, d->cin_pad);
  FArgs k{};
  k.x = d->x; k.inv_scale = d->wpack; k.wimg = reinterpret_cast<const char*>(d->wpack + 32);
  k.bias = d->bias; k.res = d->res; k.y_raw = d->y_raw;
  k.N = d->n; k.H = d->h; k.W = d->w; k.Cin = d->cin_pad; k.cout = d->cout;
  k.in_act = d->in_act; k.in_slope = d->in_slope;
  k.nchw_op = d->nchw_op; k.crop_h = d->crop_h; k.crop_w = d->crop_w; k.res_sf = d->res_sf; k.clamp_lo = d->clamp_lo; k.clamp_hi = d->clamp_hi;
  k.range_flag = virnet::range_flag_ptr();
#ifdef VIRNET_F16_TIMING
  k.tlog = g_xlog;
#endif
  // only the cropped region is produced
  k.nty = (d->crop_h + EX_TH - 1) / EX_TH;
  k.ntx = (d->crop_w + EX_TW - 1) / EX_TW;
  k.ntiles = k.N * k.nty * k.ntx;
  k.tiles_per_xcd = (k.ntiles + 7) / 8;
  VIRNET_REQUIRE((unsigned long long)k.ntiles * (unsigned)(k.ntx * k.nty) < (1ull << 32), "virnet_conv_exit: %d tiles exceed the index arithmetic of one launch", k.ntiles);
  k.mg_ntx = div_magic(k.ntx);
  k.mg_tpi = div_magic(k.ntx * k.nty);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nch = d->cin_pad >> 4;
  if (with_z) {
    VIRNET_REQUIRE(z_add != nullptr, "virnet_conv_exit_add: z_add is NULL");
    VIRNET_REQUIRE(nch == 6 || nch == 4, "virnet_conv_exit_add: cin_pad=%d (the additive map is built for 96 and 64 input channels)", d->cin_pad);
    VIRNET_REQUIRE(!d->in_act, "virnet_conv_exit_add: no input activation (z_add is linear in x only without one)");
    return nch == 6 ? launch_exit_zadd<6>(k, z_add, st) : launch_exit_zadd<4>(k, z_add, st);
  }
  if (nch == 6) return launch_exit<6>(k, st);
  if (nch == 4) return launch_exit<4>(k, st);
  VIRNET_REQUIRE(nch * 2048 + 33 * EX_ZS * 4 <= 160 * 1024, "virnet_conv_exit: cin_pad=%d does not fit LDS", d->cin_pad);
  return launch_exit<0>(k, st);
}

extern "C" int virnet_conv_exit(const virnet_conv_desc* d, void* stream) { return conv_exit_host(d, nullptr, false, stream); }

extern "C" int virnet_conv_exit_add(const virnet_conv_desc* d, const float* z_add, void* stream) { return conv_exit_host(d, z_add, true, stream); }
