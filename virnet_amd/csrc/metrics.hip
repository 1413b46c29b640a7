// metrics.hip -- uint8 PSNR / SSIM of the evaluation tables on the device (host definition: virnet_amd/eval.py; reference:
// utils/util_image.py:17-89,129-153 and skimage's img_as_ubyte).
//
//   quantize_kernel   float32 -> uint8, bit for bit eval.img_as_ubyte: clamp to [0,1] in fp32, (double)x * 255.0 (exact: 24 x 8 bits),
//                     round half to even.  NaN -> 0.
//   luma_kernel       uint8 RGB -> uint8 Y, eval.rgb2y_uint8 as the fused chain fma(b, c2, fma(g, c1, r*c0)) + 16.0 (the order matters on
//                     the 194 RGB triples whose exact value ends in .5).
//   luma_float_u8     ycbcr = 2: float32 RGB -> the Y channel in fp32 (x*255, three products, two sums, +16, /255, each rounded on its own),
//                     clamped and quantised afterwards -- the training scripts' test stage (metrics.rgb2y_float_np).
//   psnr_ssim_kernel  one workgroup per 32 x 32 tile of the SSIM map per (image, metric channel): both images' 42 x 42 input patch goes
//                     to LDS as bytes (quantised / converted to Y while it is loaded), an 11-tap horizontal pass writes the five
//                     quantities (a, b, a^2, b^2, ab) to LDS in fp64, a vertical pass (4 outputs per thread from 14 reads per
//                     quantity) gives the SSIM value per pixel.  The squared error is summed in integers over the pixels a tile OWNS
//                     (its 32 x 32 core; the last tile of a row / column also owns the remaining <= 10 columns / rows).  One fp64 and
//                     one 64-bit integer partial per workgroup, ordinary stores.
//   finish_kernel     one workgroup per image adds the partials in a fixed order: no floating-point atomics anywhere, so the result is
//                     bitwise reproducible and an image gives the same bits alone and inside a batch.
//
// Everything that decides a rounding is fp64 or integer; contraction is off for the whole unit so that every fused operation below is
// one that is written as fma().
#include "common.h"
#include "quantize.h"
#include "../../include/virnet_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWin = 11;                   // Gaussian window
constexpr int kTile = 32;                  // SSIM-map tile edge
constexpr int kIn = kTile + kWin - 1;      // 42: input patch edge
constexpr int kInPitch = 48;               // bytes per patch row: a group of four output columns reads 16 bytes from a 4-byte boundary
constexpr int kRowGroups = kTile / 4;      // 8 four-column groups per patch row

struct Window { double w[kWin]; };

using virnet::quant_u8;             // quantize.h: shared with ensemble.hip

__device__ __forceinline__ unsigned luma_u8(unsigned r, unsigned g, unsigned b) {
  constexpr double c0 = 65.481 / 255.0, c1 = 128.553 / 255.0, c2 = 24.966 / 255.0;
  const double y = fma((double)b, c2, fma((double)g, c1, (double)r * c0)) + 16.0;
  return (unsigned)(int)rint(y);
}

// ycbcr = 2: the Y channel of the FLOAT image in fp32, quantised afterwards (the training scripts' test stage: util_image.batch_PSNR
// (..., ycbcr=True) -> rgb2ycbcrTorch :155-176).  Every product, sum and the division rounds to fp32 on its own (contraction is off);
// the host definition is metrics.rgb2y_float_np.
__device__ __forceinline__ unsigned luma_float_u8(float r, float g, float b) {
  constexpr float k0 = 65.481f / 255.0f, k1 = 128.553f / 255.0f, k2 = 24.966f / 255.0f;
  const float tr = r * 255.0f, tg = g * 255.0f, tb = b * 255.0f;
  const float p0 = tr * k0, p1 = tg * k1, p2 = tb * k2;
  const float y = (((p0 + p1) + p2) + 16.0f) / 255.0f;
  return quant_u8(y);
}

__global__ __launch_bounds__(kThreads) void quantize_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, size_t n) {
  const size_t quads = n >> 2;
  const size_t stride = (size_t)gridDim.x * kThreads;
  const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if ((((uintptr_t)x & 15) | ((uintptr_t)out & 3)) == 0) {
    for (size_t i = t; i < quads; i += stride) {
      const float4 v = reinterpret_cast<const float4*>(x)[i];
      const unsigned p = quant_u8(v.x) | (quant_u8(v.y) << 8) | (quant_u8(v.z) << 16) | (quant_u8(v.w) << 24);
      reinterpret_cast<unsigned*>(out)[i] = p;
    }
    for (size_t i = (quads << 2) + t; i < n; i += stride) out[i] = (unsigned char)quant_u8(x[i]);
  } else {
    for (size_t i = t; i < n; i += stride) out[i] = (unsigned char)quant_u8(x[i]);
  }
}

__global__ __launch_bounds__(kThreads) void luma_kernel(const unsigned char* __restrict__ rgb, unsigned char* __restrict__ y, size_t hw,
                                                        size_t total) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
    const size_t n = i / hw, p = i - n * hw;
    const unsigned char* const src = rgb + n * 3 * hw + p;
    y[i] = (unsigned char)luma_u8(src[0], src[hw], src[2 * hw]);
  }
}

struct MetricArgs {
  const void* a;
  const void* b;
  double* ssim_part;               // [n][cm][tiles]
  unsigned long long* sse_part;    // [n][cm][tiles]
  int a_f32, b_f32;
  int c, h, w, border, ycbcr, with_ssim;
  int hc, wc;                      // cropped extent
  int tiles_x, tiles_y;
};

// metric value (uint8 as unsigned) of cropped pixel (y, x) of image n, metric channel ch
__device__ __forceinline__ unsigned load_px(const void* base, int f32, const MetricArgs& k, int n, int ch, int y, int x) {
  const size_t hw = (size_t)k.h * k.w;
  const size_t off = (size_t)(y + k.border) * k.w + (x + k.border);
  if (k.ycbcr) {
    const size_t o = (size_t)n * 3 * hw + off;
    unsigned r, g, b;
    if (k.ycbcr == 2) {                                       // (float32 inputs only: the host entry refuses uint8 in this mode)
      const float* const p = static_cast<const float*>(base) + o;
      return luma_float_u8(p[0], p[hw], p[2 * hw]);
    }
    if (f32) {
      const float* const p = static_cast<const float*>(base) + o;
      r = quant_u8(p[0]); g = quant_u8(p[hw]); b = quant_u8(p[2 * hw]);
    } else {
      const unsigned char* const p = static_cast<const unsigned char*>(base) + o;
      r = p[0]; g = p[hw]; b = p[2 * hw];
    }
    return luma_u8(r, g, b);
  }
  const size_t o = ((size_t)n * k.c + ch) * hw + off;
  return f32 ? quant_u8(static_cast<const float*>(base)[o]) : (unsigned)static_cast<const unsigned char*>(base)[o];
}

__global__ __launch_bounds__(kThreads) void psnr_ssim_kernel(const MetricArgs k, const Window win) {
  __shared__ __attribute__((aligned(16))) unsigned char pa[kIn * kInPitch];
  __shared__ __attribute__((aligned(16))) unsigned char pb[kIn * kInPitch];
  __shared__ __attribute__((aligned(16))) double hq[5][kIn][kTile];
  __shared__ double red_d[kThreads / 64];
  __shared__ unsigned long long red_u[kThreads / 64];

  const int tid = threadIdx.x;
  const int tile = blockIdx.x, ch = blockIdx.y, n = blockIdx.z;
  const int ty = tile / k.tiles_x, tx = tile - ty * k.tiles_x;
  const int y0 = ty * kTile, x0 = tx * kTile;
  const bool last_y = ty == k.tiles_y - 1, last_x = tx == k.tiles_x - 1;

  // ---- load both patches (zeros beyond the cropped image: they only reach SSIM positions that are masked off below) + squared error
  unsigned sse = 0;                                           // <= 8 pixels per thread x 65025
  for (int i = tid; i < kIn * kInPitch; i += kThreads) {
    const int ly = i / kInPitch, lx = i - ly * kInPitch;
    const int y = y0 + ly, x = x0 + lx;
    unsigned va = 0, vb = 0;
    if (lx < kIn && y < k.hc && x < k.wc) {
      va = load_px(k.a, k.a_f32, k, n, ch, y, x);
      vb = load_px(k.b, k.b_f32, k, n, ch, y, x);
      if ((ly < kTile || last_y) && (lx < kTile || last_x)) {
        const int d = (int)va - (int)vb;
        sse += (unsigned)(d * d);
      }
    }
    pa[i] = (unsigned char)va;
    pb[i] = (unsigned char)vb;
  }
  __syncthreads();

  double acc = 0.0;
  if (k.with_ssim) {
    // ---- horizontal pass: item = (patch row, group of four output columns); 14 input columns of both images -> 4 x 5 sums
    for (int item = tid; item < kIn * kRowGroups; item += kThreads) {
      const int row = item >> 3, cg = item & 7;
      const unsigned* const qa = reinterpret_cast<const unsigned*>(pa + row * kInPitch + cg * 4);     // 4-byte aligned
      const unsigned* const qb = reinterpret_cast<const unsigned*>(pb + row * kInPitch + cg * 4);
      const unsigned wa[4] = {qa[0], qa[1], qa[2], qa[3]}, wb[4] = {qb[0], qb[1], qb[2], qb[3]};
      double a[14], b[14];
#pragma unroll
      for (int j = 0; j < 14; ++j) {
        a[j] = (double)((wa[j >> 2] >> ((j & 3) * 8)) & 0xffu);
        b[j] = (double)((wb[j >> 2] >> ((j & 3) * 8)) & 0xffu);
      }
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        double v[14];
#pragma unroll
        for (int j = 0; j < 14; ++j) v[j] = q == 0 ? a[j] : q == 1 ? b[j] : q == 2 ? a[j] * a[j] : q == 3 ? b[j] * b[j] : a[j] * b[j];
        double o[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          double t = win.w[0] * v[s];
#pragma unroll
          for (int j = 1; j < kWin; ++j) t = fma(win.w[j], v[s + j], t);
          o[s] = t;
        }
        double2* const dst = reinterpret_cast<double2*>(&hq[q][row][cg * 4]);
        dst[0] = make_double2(o[0], o[1]);
        dst[1] = make_double2(o[2], o[3]);
      }
    }
    __syncthreads();

    // ---- vertical pass: thread = (column, group of four output rows)
    const int col = tid & (kTile - 1), r0 = (tid >> 5) * 4;
    double f[5][4];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      double v[14];
#pragma unroll
      for (int j = 0; j < 14; ++j) v[j] = hq[q][r0 + j][col];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        double t = win.w[0] * v[s];
#pragma unroll
        for (int j = 1; j < kWin; ++j) t = fma(win.w[j], v[s + j], t);
        f[q][s] = t;
      }
    }
    constexpr double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
    const bool col_ok = x0 + col < k.wc - (kWin - 1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const double mu1 = f[0][s], mu2 = f[1][s];
      const double m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
      const double s1 = f[2][s] - m11, s2 = f[3][s] - m22, s12 = f[4][s] - m12;
      const double v = ((2 * m12 + C1) * (2 * s12 + C2)) / ((m11 + m22 + C1) * (s1 + s2 + C2));
      if (col_ok && y0 + r0 + s < k.hc - (kWin - 1)) acc += v;
    }
  }

  // ---- workgroup reduction in a fixed order: lanes by halving strides, then the four waves in order
  unsigned long long sse64 = sse;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc += __shfl_down(acc, off, 64);
    sse64 += __shfl_down(sse64, off, 64);
  }
  if ((tid & 63) == 0) {
    red_d[tid >> 6] = acc;
    red_u[tid >> 6] = sse64;
  }
  __syncthreads();
  if (tid == 0) {
    const size_t slot = ((size_t)n * gridDim.y + ch) * gridDim.x + tile;
    k.ssim_part[slot] = ((red_d[0] + red_d[1]) + red_d[2]) + red_d[3];
    k.sse_part[slot] = red_u[0] + red_u[1] + red_u[2] + red_u[3];
  }
}

// one workgroup per image: thread t adds partials t, t + 256, ... of a channel in index order, then a fixed tree over the threads
__global__ __launch_bounds__(kThreads) void finish_kernel(const double* __restrict__ ssim_part, const unsigned long long* __restrict__ sse_part,
                                                          int cm, int tiles, long long map_count, long long count, int with_ssim,
                                                          long long* __restrict__ sse_out, long long* __restrict__ count_out,
                                                          double* __restrict__ ssim_out) {
  __shared__ double sd[kThreads];
  __shared__ unsigned long long su[kThreads];
  const int tid = threadIdx.x, n = blockIdx.x;
  unsigned long long sse = 0;
  double chan_mean[3] = {0.0, 0.0, 0.0};
  for (int ch = 0; ch < cm; ++ch) {
    const size_t base = ((size_t)n * cm + ch) * tiles;
    double d = 0.0;
    for (int t = tid; t < tiles; t += kThreads) {
      d += ssim_part[base + t];
      sse += sse_part[base + t];
    }
    sd[tid] = d;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
      if (tid < off) sd[tid] += sd[tid + off];
      __syncthreads();
    }
    chan_mean[ch] = sd[0] / (double)map_count;
    __syncthreads();
  }
  su[tid] = sse;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (tid < off) su[tid] += su[tid + off];
    __syncthreads();
  }
  if (tid == 0) {
    sse_out[n] = (long long)su[0];
    count_out[n] = count;
    // eval.calculate_ssim: np.mean over the channels of the per-channel map means
    const double m = cm == 3 ? ((chan_mean[0] + chan_mean[1]) + chan_mean[2]) / 3.0 : chan_mean[0];
    ssim_out[n] = with_ssim ? m : __longlong_as_double(0x7ff8000000000000ll);
  }
}

int grid_for(size_t items) {
  const size_t blocks = (items + kThreads - 1) / kThreads;
  return (int)(blocks > 16384 ? 16384 : (blocks ? blocks : 1));
}

struct Geometry { int hc, wc, cm, tiles_x, tiles_y; };

// 0 on success; the SSIM map of the cropped image is (hc - 10) x (wc - 10), tiled 32 x 32 (at least one tile so that a PSNR-only call on
// a cropped image under 11 pixels is still covered: a tile's patch reaches 42 pixels)
int geometry(int n, int c, int h, int w, int border, int ycbcr, int with_ssim, Geometry* g) {
  VIRNET_REQUIRE(n > 0 && n <= 65535, "virnet_psnr_ssim: batch %d outside 1..65535", n);
  VIRNET_REQUIRE(c == 1 || c == 3, "virnet_psnr_ssim: %d channels (1 or 3 expected)", c);
  VIRNET_REQUIRE(ycbcr >= 0 && ycbcr <= 2, "virnet_psnr_ssim: ycbcr=%d (0 = channels, 1 = Y of the uint8 image, 2 = Y of the float image)", ycbcr);
  VIRNET_REQUIRE(!ycbcr || c == 3, "virnet_psnr_ssim: ycbcr needs 3 channels, got %d", c);
  VIRNET_REQUIRE(border >= 0, "virnet_psnr_ssim: negative border %d", border);
  VIRNET_REQUIRE(h > 0 && w > 0 && h <= (1 << 24) && w <= (1 << 24) && border < (1 << 23), "virnet_psnr_ssim: bad size %dx%d border %d", h, w,
                 border);
  const int need = (with_ssim ? kWin : 1) + 2 * border;
  VIRNET_REQUIRE(h >= need && w >= need, "virnet_psnr_ssim: %dx%d with border %d is smaller than %d pixels", h, w, border, need);
  g->hc = h - 2 * border;
  g->wc = w - 2 * border;
  g->cm = ycbcr ? 1 : c;
  const int mh = g->hc - (kWin - 1), mw = g->wc - (kWin - 1);
  g->tiles_y = mh > 0 ? (mh + kTile - 1) / kTile : 1;
  g->tiles_x = mw > 0 ? (mw + kTile - 1) / kTile : 1;
  return 0;
}

}  // namespace

extern "C" int virnet_quantize_u8(const float* x, uint8_t* out, size_t n, void* stream) {
  VIRNET_REQUIRE(x && out, "virnet_quantize_u8: NULL pointer");
  VIRNET_REQUIRE(n > 0, "virnet_quantize_u8: empty tensor");
  hipLaunchKernelGGL(quantize_kernel, dim3(grid_for((n + 3) / 4)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), x, out, n);
  return virnet::check_launch("quantize launch");
}

extern "C" int virnet_rgb2y_u8(const uint8_t* rgb, uint8_t* y, int n, int h, int w, void* stream) {
  VIRNET_REQUIRE(rgb && y, "virnet_rgb2y_u8: NULL pointer");
  VIRNET_REQUIRE(n > 0 && h > 0 && w > 0, "virnet_rgb2y_u8: bad shape n=%d h=%d w=%d", n, h, w);
  const size_t hw = (size_t)h * w, total = hw * n;
  hipLaunchKernelGGL(luma_kernel, dim3(grid_for(total)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), rgb, y, hw, total);
  return virnet::check_launch("luma launch");
}

extern "C" size_t virnet_psnr_ssim_workspace_bytes(int n, int c, int h, int w, int border, int ycbcr) {
  Geometry g;
  if (geometry(n, c, h, w, border, ycbcr, 0, &g)) return 0;
  return (size_t)n * g.cm * g.tiles_x * g.tiles_y * (sizeof(double) + sizeof(unsigned long long));
}

extern "C" int virnet_psnr_ssim(const void* a, int a_f32, const void* b, int b_f32, int n, int c, int h, int w, int border, int ycbcr,
                                int with_ssim, const double* win11, void* workspace, int64_t* sse, int64_t* count, double* ssim,
                                void* stream) {
  VIRNET_REQUIRE(a && b && workspace && sse && count && ssim, "virnet_psnr_ssim: NULL pointer");
  VIRNET_REQUIRE(!with_ssim || win11, "virnet_psnr_ssim: NULL window");
  VIRNET_REQUIRE(((uintptr_t)workspace & 7) == 0, "virnet_psnr_ssim: workspace must be 8-byte aligned");
  VIRNET_REQUIRE((!a_f32 || ((uintptr_t)a & 3) == 0) && (!b_f32 || ((uintptr_t)b & 3) == 0), "virnet_psnr_ssim: misaligned float32 image");
  VIRNET_REQUIRE(ycbcr != 2 || (a_f32 && b_f32), "virnet_psnr_ssim: ycbcr=2 (Y of the float image) needs float32 inputs");
  Geometry g;
  if (geometry(n, c, h, w, border, ycbcr, with_ssim, &g)) return 1;
  const long long tiles = (long long)g.tiles_x * g.tiles_y;
  VIRNET_REQUIRE(tiles <= (1ll << 30), "virnet_psnr_ssim: %dx%d is too large (%lld tiles)", h, w, tiles);
  MetricArgs k;
  k.a = a; k.b = b;
  k.ssim_part = static_cast<double*>(workspace);
  k.sse_part = reinterpret_cast<unsigned long long*>(k.ssim_part + (size_t)n * g.cm * tiles);
  k.a_f32 = a_f32 != 0; k.b_f32 = b_f32 != 0;
  k.c = c; k.h = h; k.w = w; k.border = border; k.ycbcr = ycbcr; k.with_ssim = with_ssim != 0;
  k.hc = g.hc; k.wc = g.wc; k.tiles_x = g.tiles_x; k.tiles_y = g.tiles_y;
  Window win;
  for (int i = 0; i < kWin; ++i) win.w[i] = with_ssim ? win11[i] : 0.0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(psnr_ssim_kernel, dim3((unsigned)tiles, g.cm, n), dim3(kThreads), 0, s, k, win);
  if (int rc = virnet::check_launch("psnr_ssim launch")) return rc;
  const long long map_count = with_ssim ? (long long)(g.hc - (kWin - 1)) * (g.wc - (kWin - 1)) : 1;
  const long long cnt = (long long)g.hc * g.wc * g.cm;
  hipLaunchKernelGGL(finish_kernel, dim3(n), dim3(kThreads), 0, s, k.ssim_part, k.sse_part, g.cm, (int)tiles, map_count, cnt, k.with_ssim,
                     reinterpret_cast<long long*>(sse), reinterpret_cast<long long*>(count), ssim);
  return virnet::check_launch("psnr_ssim finish launch");
}
