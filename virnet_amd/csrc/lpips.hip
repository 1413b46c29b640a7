// lpips.hip -- LPIPS v0.1 (net = 'alex', spatial = False, eval mode) of the SISR evaluation table on the device (host definition:
// virnet_amd/lpips.py distance_torch; reference: scripts/sisr_virnet_syn.py:158-161 with utils/util_image.py:118-126).
//
// Both images of a pair go through the feature stack as ONE batch of 2n (a's images first), in fp32 NHWC:
//
//   lpips_stem_kernel      conv1 (3 -> 64, 11 x 11, stride 4, pad 2) + ReLU.  One workgroup per 8 x 8 output pixels of an image: the 39 x 39 x 3
//                          input patch goes to LDS already quantised (uint8, or float32 through quant_u8), mapped to [-1, 1] and through
//                          the scaling layer; a tap outside the image is 0 AFTER the scaling, as the padded convolution sees it.  A wave owns
//                          16 output channels (its weights are wave-uniform) and a lane one pixel: 363 x 16 fmaf per lane, k ascending.
//   lpips_pool_kernel      3 x 3 / stride 2 max-pool without padding (every window lies inside the map).
//   lpips_conv_kernel<KS>  conv2..5 as an implicit GEMM on the exact-f32 matrix instruction v_mfma_f32_32x32x2_f32: M = flat pixel index
//                          over the whole batch, N = output channel, K = (ky, kx, c).  The deep maps are small (29 x 19 for a 480 x 320
//                          image), so the work is cut fine: a workgroup owns one 32 pixel x 32 channel tile and deals the K steps (the 32
//                          channels of one tap) to its four waves in turn; operands go from global memory straight to registers, the next
//                          step's loads in flight, and nothing synchronises until the four sums are added in wave order.  A step is one
//                          k-ordered fmaf chain from zero: the same sums for every output wherever its tile lies, with the rounding error
//                          of blocked summation.
//   lpips_score_kernel     all five taps in one launch.  A wave takes one pixel at a time: both channel norms, then
//                          sum_c w_c (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2, in fp64, lanes joined by a butterfly (every lane holds the
//                          same bits, and swapping the two images changes no bit).  One fp64 partial per workgroup, ordinary stores.
//   lpips_finish_kernel    one workgroup per pair adds the partials of each tap in a fixed order, divides by the tap's pixel count and adds
//                          the five means in tap order.
//   lpips_nchw_kernel      NHWC -> NCHW copy of a tap (virnet_lpips_features only).
//
// No atomics, no allocation, no synchronisation; all scratch lies in the caller's workspace.
#include "common.h"
#include "quantize.h"
#include "../../include/virnet_hip.h"

#include <cstdint>

// every fused operation below is one that is written as fma(): a contracted x0 * r0 - x1 * r1 would be neither symmetric nor 0 for equal images
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTaps = 5;
constexpr int kChan[kTaps] = {64, 192, 384, 256, 256};

using virnet::quant_u8;
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- geometry --------------------------------------------------------------------------------------------------------------------------
constexpr int kStemTile = 8;                              // output pixels per workgroup edge
constexpr int kStemIn = (kStemTile - 1) * 4 + 11;         // 39: input patch edge
constexpr int kStemPitch = 40;
constexpr int kScorePix = 64;                             // pixels per score workgroup

struct Geometry {
  int images, pairs;
  int h[3], w[3];                  // conv1 map, first pool, second pool
  long long pix[kTaps];            // pixels per image of every tap
  size_t off[7];                   // float offsets in the workspace: relu1, pool1, relu2, pool2, relu3, relu4, relu5
  size_t part_off;                 // byte offset of the fp64 partials
  int blk0[kTaps + 1];             // first score workgroup of every tap (per pair)
  size_t bytes;
};

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int geometry(const char* who, int images, int pairs, int h, int w, Geometry* g) {
  VIRNET_REQUIRE(images > 0 && images <= 65534 && pairs >= 0 && pairs <= 32767, "%s: batch %d outside 1..32767", who, pairs ? pairs : images);
  VIRNET_REQUIRE(h >= 31 && w >= 31, "%s: %dx%d is smaller than 31x31, the smallest image both max-pools accept", who, h, w);
  VIRNET_REQUIRE(h <= (1 << 20) && w <= (1 << 20), "%s: bad size %dx%d", who, h, w);
  g->images = images;
  g->pairs = pairs;
  g->h[0] = (h - 7) / 4 + 1;
  g->w[0] = (w - 7) / 4 + 1;
  for (int i = 1; i < 3; ++i) {
    g->h[i] = (g->h[i - 1] - 3) / 2 + 1;
    g->w[i] = (g->w[i - 1] - 3) / 2 + 1;
  }
  const long long p1 = (long long)g->h[0] * g->w[0], p2 = (long long)g->h[1] * g->w[1], p3 = (long long)g->h[2] * g->w[2];
  g->pix[0] = p1; g->pix[1] = p2; g->pix[2] = g->pix[3] = g->pix[4] = p3;
  const long long elems[8] = {images * p1 * kChan[0], images * p2 * kChan[0], images * p2 * kChan[1], images * p3 * kChan[1],
                              images * p3 * kChan[2], images * p3 * kChan[3], images * p3 * kChan[4], (long long)images * 3 * h * w};
  for (int i = 0; i < 8; ++i)
    VIRNET_REQUIRE(elems[i] < (1ll << 31), "%s: %d images of %dx%d need a tensor of %lld elements (limit 2^31 - 1)", who, images, h, w, elems[i]);
  size_t at = 0;
  for (int i = 0; i < 7; ++i) {
    g->off[i] = at;
    at += round_up((size_t)elems[i], 64);
  }
  g->part_off = at * sizeof(float);
  int blk = 0;
  for (int i = 0; i < kTaps; ++i) {
    g->blk0[i] = blk;
    blk += (int)((g->pix[i] + kScorePix - 1) / kScorePix);
  }
  g->blk0[kTaps] = blk;
  g->bytes = g->part_off + (size_t)pairs * blk * sizeof(double);
  return 0;
}

// ---- conv1 -----------------------------------------------------------------------------------------------------------------------------
struct StemArgs {
  const void* a;                   // images 0 .. n - 1
  const void* b;                   // images n .. 2n - 1 (unused when the batch is a alone)
  const float* wt;                 // [363][64], k = (c * 11 + ky) * 11 + kx
  const float* bias;
  float* out;                      // [images][h1][w1][64]
  int a_f32, b_f32, n, h, w, h1, w1, tiles_x;
  float shift[3], scale[3];
};

__global__ __launch_bounds__(kThreads) void lpips_stem_kernel(const StemArgs k) {
  __shared__ float patch[3 * kStemIn * kStemPitch];
  const int tid = threadIdx.x;
  const int img = blockIdx.y;
  const int ty = blockIdx.x / k.tiles_x, tx = blockIdx.x - ty * k.tiles_x;
  const int oy0 = ty * kStemTile, ox0 = tx * kStemTile;
  const int iy0 = oy0 * 4 - 2, ix0 = ox0 * 4 - 2;
  const bool second = img >= k.n;
  const void* const src = second ? k.b : k.a;
  const int f32 = second ? k.b_f32 : k.a_f32;
  const size_t hw = (size_t)k.h * k.w;
  const size_t base = (size_t)(second ? img - k.n : img) * 3 * hw;

  for (int i = tid; i < 3 * kStemIn * kStemPitch; i += kThreads) {
    const int c = i / (kStemIn * kStemPitch), r = i - c * (kStemIn * kStemPitch);
    const int ly = r / kStemPitch, lx = r - ly * kStemPitch;
    const int y = iy0 + ly, x = ix0 + lx;
    float v = 0.f;
    if (lx < kStemIn && y >= 0 && y < k.h && x >= 0 && x < k.w) {
      const size_t o = base + c * hw + (size_t)y * k.w + x;
      const unsigned u = f32 ? quant_u8(static_cast<const float*>(src)[o]) : (unsigned)static_cast<const unsigned char*>(src)[o];
      const float xn = ((float)u - 127.5f) / 127.5f;
      const float sh = c == 0 ? k.shift[0] : c == 1 ? k.shift[1] : k.shift[2];
      const float sc = c == 0 ? k.scale[0] : c == 1 ? k.scale[1] : k.scale[2];
      v = (xn - sh) / sc;
    }
    patch[i] = v;
  }
  __syncthreads();

  const int p = tid & 63, py = p >> 3, px = p & 7;
  const int cg = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float* const wp = k.wt + cg * 16;
  float acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = k.bias[cg * 16 + j];
  for (int c = 0; c < 3; ++c) {
    for (int ky = 0; ky < 11; ++ky) {
      const float* const row = patch + (c * kStemIn + py * 4 + ky) * kStemPitch + px * 4;
      const float* const wr = wp + (size_t)((c * 11 + ky) * 11) * 64;
#pragma unroll
      for (int kx = 0; kx < 11; ++kx) {
        const float v = row[kx];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = fmaf(v, wr[kx * 64 + j], acc[j]);
      }
    }
  }
  const int oy = oy0 + py, ox = ox0 + px;
  if (oy < k.h1 && ox < k.w1) {
    float4* const dst = reinterpret_cast<float4*>(k.out + (((size_t)img * k.h1 + oy) * k.w1 + ox) * 64 + cg * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      dst[q] = make_float4(fmaxf(acc[q * 4], 0.f), fmaxf(acc[q * 4 + 1], 0.f), fmaxf(acc[q * 4 + 2], 0.f), fmaxf(acc[q * 4 + 3], 0.f));
  }
}

// ---- max-pool --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 max4(float4 a, float4 b) {
  return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}

// in [images][hi][wi][4 c4] -> out [images][ho][wo][4 c4], ho = (hi - 3) / 2 + 1: row 2 (ho - 1) + 2 <= hi - 1
__global__ __launch_bounds__(kThreads) void lpips_pool_kernel(const float4* __restrict__ in, float4* __restrict__ out, int hi, int wi, int ho, int wo,
                                                              int c4, size_t total) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
    const int q = (int)(i % c4);
    size_t t = i / c4;
    const int x = (int)(t % wo);
    t /= wo;
    const int y = (int)(t % ho);
    const size_t b = t / ho;
    const float4* const src = in + ((b * hi + 2 * y) * wi + 2 * x) * c4 + q;
    float4 m = src[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx)
        if (dy | dx) m = max4(m, src[((size_t)dy * wi + dx) * c4]);
    out[i] = m;
  }
}

// ---- conv2..5 --------------------------------------------------------------------------------------------------------------------------
constexpr int kBM = 32, kBN = 32, kBK = 32;      // a workgroup owns ONE 32 x 32 tile of the matrix instruction; a K step is 32 channels of a tap
constexpr int kSplit = kThreads / 64;            // the K steps are dealt to the four waves in turn (wave v takes steps v, v + 4, ...)

struct ConvArgs {
  const float* x;                  // [images][H][W][cin]
  const float* w;                  // [KS * KS * cin][cout], k = (ky * KS + kx) * cin + c
  const float* bias;
  float* y;                        // [images][H][W][cout], after ReLU
  int m, h, w_, cin, cout;         // m = images * H * W
};

template <int KS>
__global__ __launch_bounds__(kThreads) void lpips_conv_kernel(const ConvArgs k) {
  __shared__ float red[kSplit][16][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 31, half = lane >> 5;
  const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * kBN;

  // operands straight from global memory, no LDS: lane (i, half) holds pixel m0 + i as the A row and output channel n0 + i as the B
  // column; within a K step it takes channels half * 16 .. + 15, so instruction kk of the step multiplies channels kk and 16 + kk
  const int am = m0 + i;
  const bool a_ok = am < k.m;
  const int hw = k.h * k.w_;
  const int ab = am / hw, ar = am - ab * hw;
  const int ay = ar / k.w_, ax = ar - ay * k.w_;
  const float* const wcol = k.w + n0 + i;

  const int csteps = k.cin / kBK, nsteps = KS * KS * csteps;
  float na[16], nb[16];
  auto fetch = [&](int s) {
    const int tap = s / csteps, c0 = (s - tap * csteps) * kBK + half * 16;
    const int ky = tap / KS, kx = tap - ky * KS;
    const int yy = ay + ky - KS / 2, xx = ax + kx - KS / 2;
    const bool ok = a_ok && yy >= 0 && yy < k.h && xx >= 0 && xx < k.w_;
    const float4* const p = reinterpret_cast<const float4*>(k.x + (((size_t)ab * k.h + yy) * k.w_ + xx) * k.cin + c0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 t = ok ? p[q] : make_float4(0.f, 0.f, 0.f, 0.f);
      na[q * 4] = t.x; na[q * 4 + 1] = t.y; na[q * 4 + 2] = t.z; na[q * 4 + 3] = t.w;
    }
    const float* const q = wcol + (size_t)(tap * k.cin + c0) * k.cout;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) nb[kk] = q[(size_t)kk * k.cout];
  };

  // a step is one k-ordered fmaf chain from zero (inside the matrix instruction); a wave adds its steps in order
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if (wave < nsteps) fetch(wave);
  for (int s = wave; s < nsteps; s += kSplit) {
    float ca[16], cb[16];
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      ca[kk] = na[kk];
      cb[kk] = nb[kk];
    }
    if (s + kSplit < nsteps) fetch(s + kSplit);
    f32x16 blk;
#pragma unroll
    for (int r = 0; r < 16; ++r) blk[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) blk = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[kk], cb[kk], blk, 0, 0, 0);
    acc += blk;
  }

  // the four waves' sums are added in wave order.  D[i][j]: j = lane & 31 (output channel), i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (pixel)
#pragma unroll
  for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
  __syncthreads();
  const int co = n0 + i;
  const float bias = k.bias[co];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = wave * 4 + q;
    const float v = ((red[0][r][lane] + red[1][r][lane]) + red[2][r][lane]) + red[3][r][lane];
    const int m = m0 + q + 8 * wave + 4 * half;
    if (m < k.m) k.y[(size_t)m * k.cout + co] = fmaxf(v + bias, 0.f);
  }
}

// ---- score -----------------------------------------------------------------------------------------------------------------------------
struct ScoreArgs {
  const float* feat[kTaps];        // [2 pairs][pix][C]
  const float* lin[kTaps];         // [C]
  int chan[kTaps];
  int pix[kTaps];
  int blk0[kTaps + 1];
  int pairs;
  double* part;                    // [pairs][blk0[5]]
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(kThreads) void lpips_score_kernel(const ScoreArgs k) {
  __shared__ double red[kThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blk = blockIdx.x, n = blockIdx.y;
  const float* f = k.feat[0];
  const float* lw = k.lin[0];
  int chan = k.chan[0], pix = k.pix[0], b0 = 0;
#pragma unroll
  for (int i = 1; i < kTaps; ++i)
    if (blk >= k.blk0[i]) {
      f = k.feat[i]; lw = k.lin[i]; chan = k.chan[i]; pix = k.pix[i]; b0 = k.blk0[i];
    }
  float wl[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) wl[i] = i * 64 < chan ? lw[i * 64 + lane] : 0.f;

  double total = 0.0;
  const int p0 = (blk - b0) * kScorePix;
  for (int j = wave; j < kScorePix; j += kThreads / 64) {
    const int p = p0 + j;
    if (p >= pix) break;
    const float* const f0 = f + ((size_t)n * pix + p) * chan;
    const float* const f1 = f + ((size_t)(k.pairs + n) * pix + p) * chan;
    float v0[6], v1[6];
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      v0[i] = v1[i] = 0.f;
      if (i * 64 < chan) {
        v0[i] = f0[i * 64 + lane];
        v1[i] = f1[i * 64 + lane];
      }
      s0 = fma((double)v0[i], (double)v0[i], s0);
      s1 = fma((double)v1[i], (double)v1[i], s1);
    }
    const double r0 = 1.0 / (sqrt(wave_sum(s0)) + 1e-10), r1 = 1.0 / (sqrt(wave_sum(s1)) + 1e-10);
    double d = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double e = (double)v0[i] * r0 - (double)v1[i] * r1;
      d = fma((double)wl[i] * e, e, d);
    }
    total += wave_sum(d);
  }
  if (lane == 0) red[wave] = total;
  __syncthreads();
  if (tid == 0) k.part[(size_t)n * k.blk0[kTaps] + blk] = ((red[0] + red[1]) + red[2]) + red[3];
}

struct FinishArgs {
  const double* part;
  double* out;
  int blk0[kTaps + 1];
  int pix[kTaps];
};

// one workgroup per pair: thread t adds partials t, t + 256, ... of a tap in index order, then a fixed tree over the threads
__global__ __launch_bounds__(kThreads) void lpips_finish_kernel(const FinishArgs k) {
  __shared__ double sd[kThreads];
  const int tid = threadIdx.x, n = blockIdx.x;
  const double* const part = k.part + (size_t)n * k.blk0[kTaps];
  double result = 0.0;
#pragma unroll
  for (int l = 0; l < kTaps; ++l) {
    double d = 0.0;
    for (int t = k.blk0[l] + tid; t < k.blk0[l + 1]; t += kThreads) d += part[t];
    sd[tid] = d;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
      if (tid < off) sd[tid] += sd[tid + off];
      __syncthreads();
    }
    result += sd[0] / (double)k.pix[l];
    __syncthreads();
  }
  if (tid == 0) k.out[n] = result;
}

// ---- NHWC -> NCHW ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void lpips_nchw_kernel(const float* __restrict__ in, float* __restrict__ out, int chan, size_t pix, size_t total) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
    const size_t p = i % pix, t = i / pix;
    const size_t c = t % chan, b = t / chan;
    out[i] = in[(b * pix + p) * chan + c];
  }
}

int grid_for(size_t items) {
  const size_t blocks = (items + kThreads - 1) / kThreads;
  return (int)(blocks > 16384 ? 16384 : (blocks ? blocks : 1));
}

int check_weights(const char* who, const virnet_lpips_weights* wts) {
  VIRNET_REQUIRE(wts, "%s: NULL weights", who);
  for (int i = 0; i < kTaps; ++i) {
    VIRNET_REQUIRE(wts->conv_w[i] && wts->conv_b[i] && wts->lin[i], "%s: NULL weight pointer of stage %d", who, i + 1);
    VIRNET_REQUIRE(((uintptr_t)wts->conv_w[i] & 15) == 0, "%s: the packed weight of conv%d is not 16-byte aligned", who, i + 1);
  }
  return 0;
}

// the feature stack of g.images images (a's n first, then b's when b is given): relu1..5 land at g.off[0], [2], [4], [5], [6] of the workspace
int run_stack(const void* a, int a_f32, const void* b, int b_f32, int n, int h, int w, const Geometry& g, const virnet_lpips_weights* wts,
              float* ws, hipStream_t s) {
  StemArgs st;
  st.a = a; st.b = b; st.wt = wts->conv_w[0]; st.bias = wts->conv_b[0]; st.out = ws + g.off[0];
  st.a_f32 = a_f32 != 0; st.b_f32 = b_f32 != 0; st.n = n; st.h = h; st.w = w; st.h1 = g.h[0]; st.w1 = g.w[0];
  st.tiles_x = (g.w[0] + kStemTile - 1) / kStemTile;
  const int tiles_y = (g.h[0] + kStemTile - 1) / kStemTile;
  for (int c = 0; c < 3; ++c) {
    st.shift[c] = wts->shift[c];
    st.scale[c] = wts->scale[c];
  }
  hipLaunchKernelGGL(lpips_stem_kernel, dim3((unsigned)(st.tiles_x * tiles_y), g.images), dim3(kThreads), 0, s, st);
  if (int rc = virnet::check_launch("lpips stem launch")) return rc;

  // stage i (1-based) 2..5: input at workspace slot src[i], output at dst[i]; a pool precedes conv2 and conv3
  const int src_slot[kTaps] = {-1, 1, 3, 4, 5}, dst_slot[kTaps] = {0, 2, 4, 5, 6};
  for (int i = 1; i < kTaps; ++i) {
    const int lvl = i < 2 ? 1 : 2;                        // map size of stage i + 1: g.h[lvl] x g.w[lvl]
    if (i <= 2) {
      const int c4 = kChan[i - 1] / 4;
      const size_t total = (size_t)g.images * g.h[lvl] * g.w[lvl] * c4;
      hipLaunchKernelGGL(lpips_pool_kernel, dim3(grid_for(total)), dim3(kThreads), 0, s, reinterpret_cast<const float4*>(ws + g.off[dst_slot[i - 1]]),
                         reinterpret_cast<float4*>(ws + g.off[src_slot[i]]), g.h[lvl - 1], g.w[lvl - 1], g.h[lvl], g.w[lvl], c4, total);
      if (int rc = virnet::check_launch("lpips pool launch")) return rc;
    }
    ConvArgs cv;
    cv.x = ws + g.off[src_slot[i]]; cv.w = wts->conv_w[i]; cv.bias = wts->conv_b[i]; cv.y = ws + g.off[dst_slot[i]];
    cv.m = (int)((long long)g.images * g.h[lvl] * g.w[lvl]); cv.h = g.h[lvl]; cv.w_ = g.w[lvl]; cv.cin = kChan[i - 1]; cv.cout = kChan[i];
    static_assert(kChan[0] % kBK == 0 && kChan[1] % kBK == 0 && kChan[2] % kBK == 0 && kChan[3] % kBK == 0, "K steps are whole");
    static_assert(kChan[1] % kBN == 0 && kChan[2] % kBN == 0 && kChan[3] % kBN == 0 && kChan[4] % kBN == 0, "channel tiles are whole");
    static_assert(kSplit == 4, "the epilogue adds four waves' sums");
    const dim3 grid((unsigned)((cv.m + kBM - 1) / kBM), (unsigned)(cv.cout / kBN));
    if (i == 1) hipLaunchKernelGGL(lpips_conv_kernel<5>, grid, dim3(kThreads), 0, s, cv);
    else hipLaunchKernelGGL(lpips_conv_kernel<3>, grid, dim3(kThreads), 0, s, cv);
    if (int rc = virnet::check_launch("lpips conv launch")) return rc;
  }
  return 0;
}

int check_images(const char* who, const void* p, int f32, const char* name) {
  VIRNET_REQUIRE(p, "%s: NULL pointer (%s)", who, name);
  VIRNET_REQUIRE(!f32 || ((uintptr_t)p & 3) == 0, "%s: misaligned float32 image (%s)", who, name);
  return 0;
}

}  // namespace

extern "C" size_t virnet_lpips_workspace_bytes(int images, int pairs, int h, int w) {
  Geometry g;
  if (geometry("virnet_lpips_workspace_bytes", images, pairs, h, w, &g)) return 0;
  return g.bytes;
}

extern "C" int virnet_lpips(const void* a, int a_f32, const void* b, int b_f32, int n, int h, int w, const virnet_lpips_weights* wts,
                            void* workspace, double* out, void* stream) {
  const char* const who = "virnet_lpips";
  if (check_images(who, a, a_f32, "a") || check_images(who, b, b_f32, "b") || check_weights(who, wts)) return 1;
  VIRNET_REQUIRE(workspace && out, "%s: NULL pointer", who);
  VIRNET_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", who);
  VIRNET_REQUIRE(n > 0 && n <= 32767, "%s: batch %d outside 1..32767", who, n);
  Geometry g;
  if (geometry(who, 2 * n, n, h, w, &g)) return 1;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* const ws = static_cast<float*>(workspace);
  if (int rc = run_stack(a, a_f32, b, b_f32, n, h, w, g, wts, ws, s)) return rc;

  const int slot[kTaps] = {0, 2, 4, 5, 6};
  ScoreArgs sc;
  FinishArgs fin;
  for (int i = 0; i < kTaps; ++i) {
    sc.feat[i] = ws + g.off[slot[i]];
    sc.lin[i] = wts->lin[i];
    sc.chan[i] = kChan[i];
    sc.pix[i] = fin.pix[i] = (int)g.pix[i];
  }
  for (int i = 0; i <= kTaps; ++i) sc.blk0[i] = fin.blk0[i] = g.blk0[i];
  sc.pairs = n;
  sc.part = reinterpret_cast<double*>(static_cast<char*>(workspace) + g.part_off);
  fin.part = sc.part;
  fin.out = out;
  hipLaunchKernelGGL(lpips_score_kernel, dim3((unsigned)g.blk0[kTaps], n), dim3(kThreads), 0, s, sc);
  if (int rc = virnet::check_launch("lpips score launch")) return rc;
  hipLaunchKernelGGL(lpips_finish_kernel, dim3(n), dim3(kThreads), 0, s, fin);
  return virnet::check_launch("lpips finish launch");
}

extern "C" int virnet_lpips_features(const void* x, int x_f32, int n, int h, int w, const virnet_lpips_weights* wts, void* workspace, float* out1,
                                     float* out2, float* out3, float* out4, float* out5, void* stream) {
  const char* const who = "virnet_lpips_features";
  if (check_images(who, x, x_f32, "x") || check_weights(who, wts)) return 1;
  VIRNET_REQUIRE(workspace && out1 && out2 && out3 && out4 && out5, "%s: NULL pointer", who);
  VIRNET_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", who);
  Geometry g;
  if (geometry(who, n, 0, h, w, &g)) return 1;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* const ws = static_cast<float*>(workspace);
  if (int rc = run_stack(x, x_f32, nullptr, 0, n, h, w, g, wts, ws, s)) return rc;
  const int slot[kTaps] = {0, 2, 4, 5, 6};
  float* const outs[kTaps] = {out1, out2, out3, out4, out5};
  for (int i = 0; i < kTaps; ++i) {
    const size_t total = (size_t)n * g.pix[i] * kChan[i];
    hipLaunchKernelGGL(lpips_nchw_kernel, dim3(grid_for(total)), dim3(kThreads), 0, s, ws + g.off[slot[i]], outs[i], kChan[i], (size_t)g.pix[i], total);
    if (int rc = virnet::check_launch("lpips nchw launch")) return rc;
  }
  return 0;
}
