// datagen.hip -- training batches synthesised on the device from a device-resident uint8 image pool (host side: virnet_amd/datagen.py;
// reference datasets/DenoisingDatasets.py:74-99, 137-155, 190-253 and datasets/SISRDatasets.py:66-104: crop, float conversion, sigma map, noise,
// eight-way augmentation, blur-kernel construction).
//
//   The pool is HWC uint8, images back to back without padding, described by a table of (byte offset, height, width) per image.  The
//   parameters of a batch of n samples are one blob of 96 n bytes, laid out as sections of n values each: eight 4-byte sections (image
//   index, crop row, crop column, augmentation flag, niid, qf as int32, std as fp32, one unused) and then eight fp64 sections (centre row,
//   centre column, 2 scale^2, down, up, lambda_1^2, lambda_2^2, theta).  The host checks their ranges before it uploads them.
//
//   datagen_patch_kernel<MODE>   one workgroup per 32 x 32 tile of OUTPUT pixels of one sample.  The augmentation maps the tile to a source
//                                rectangle of the crop (transposed for flags 2, 3, 6, 7); the workgroup stages that rectangle through LDS --
//                                pool bytes by byte loads along source rows (rows start at arbitrary byte offsets, nothing is ever read
//                                outside the crop), the noise along source rows -- and then every thread forms four neighbouring output
//                                pixels of all planes and stores them as one 16-byte store per plane (4-byte stores when the patch size is
//                                no multiple of four).  kDenoise: im_gt = u8 * fp32(1/255), sigma = the normalised Gaussian bump evaluated
//                                in fp64 without a reduction (its extremes in closed form), im_noisy = im_gt + fp32(noise * sigma) with the
//                                product and the sum rounded separately, sigma_map_gt = max(sigma^2, fp32(1e-10)).  kPair: two pools, no
//                                noise.  kHr: one pool, u8 / 255 as a true division.
//   datagen_pair_mix_kernel      kPair followed by MixUp (datasets/data_tools.py:19-30, train_denoising_real.py:160-164): the workgroup
//                                stages the tile's source rectangle of its sample and that of the same output tile of the sample's partner
//                                perm[n] (own image, crop origin and flag) from both pools -- four byte tiles -- and stores
//                                lam x + (1 - lam) x_partner, every operation rounded on its own.
//   mixup_kernel                 the same mix of two fp32 tensors already in memory: four elements per thread.
//   datagen_normal_kernel        the same generator as a fill: out[n][e] for e < per.
//   datagen_blur_kernel          one workgroup per sample: utils/util_sisr.py:60-93 in fp64 (covariance, inverse, exponent, softmax).
//
//   Noise: Philox4x32-10 keyed by the 64-bit seed, counter (e >> 2, stream, sample id low, sample id high) with e = (c P + i) P + j at
//   SOURCE coordinates; the four output words give four normals by two Box-Muller transforms with exact 24-bit uniforms, element e takes
//   normal e & 3.  A sample's noise therefore depends on its id alone, not on the batch it is in or the tile that draws it.
//
// No atomics, no scratch; contraction is off so that products and sums round where the definitions in datagen.py round them.
#include "common.h"
#include "../../include/virnet_hip.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;                        // output pixels per tile side: 32 rows x 8 threads x 4 pixels
constexpr int kRowBytes = kTile * 3 + 4;         // LDS row of staged pool bytes
constexpr int kNoiseRow = kTile + 1;             // LDS row of staged noise (odd: a walk down a column touches every bank)
constexpr int kQuads = kTile / 4 + 1;            // Philox counters that a row of kTile elements can touch when it starts mid-quad

enum Mode { kDenoise = 0, kPair = 1, kHr = 2 };

struct PatchArgs {
  const unsigned char* pool_a;
  const unsigned char* pool_b;
  const long long* table;                        // [images][3]: byte offset, height, width
  const unsigned char* params;                   // the blob described above
  const unsigned char* mix;                      // int32 perm[n], fp32 lam[n] (the pair-mix kernel only)
  const float* noise;                            // [n][3][p][p] at source coordinates, or NULL: drawn here
  const long long* sample_ids;                   // [n]
  float *out0, *out1, *out2;
  unsigned long long seed;
  unsigned stream_id;
  int n, p, tiles_x, clip, vec;
};

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&w)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// two normals of a word pair: u1 = ((a >> 8) + 1) 2^-24 in (0, 1], u2 = (b >> 8) 2^-24 in [0, 1), both exact
__device__ __forceinline__ void box_muller(unsigned a, unsigned b, float& z0, float& z1) {
  const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;
  const float u2 = (float)(b >> 8) * 0x1p-24f;
  const float r = sqrtf(-2.f * logf(u1));
  float s, c;
  sincospif(2.f * u2, &s, &c);
  z0 = r * c;
  z1 = r * s;
}

// the four normals of counter q of one sample
__device__ __forceinline__ void normals4(unsigned q, unsigned stream_id, long long sample_id, unsigned long long seed, float (&z)[4]) {
  unsigned w[4];
  philox4x32_10(q, stream_id, (unsigned)((unsigned long long)sample_id & 0xFFFFFFFFull), (unsigned)((unsigned long long)sample_id >> 32),
                (unsigned)(seed & 0xFFFFFFFFull), (unsigned)(seed >> 32), w);
  box_muller(w[0], w[1], z[0], z[1]);
  box_muller(w[2], w[3], z[2], z[3]);
}

__device__ __forceinline__ void store4(float* q, int cnt, bool vec, const float (&r)[4]) {
  if (vec) {
    *reinterpret_cast<float4*>(q) = make_float4(r[0], r[1], r[2], r[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) q[k] = r[k];
  }
}

// the bump of datasets/DenoisingDatasets.py:190-203 before its normalisation, at squared distances (di2, dj2) from the centre
__device__ __forceinline__ double bump(double di2, double dj2, double denom) { return exp((-di2 - dj2) / denom); }

// One output tile [oi0, oi1) x [oj0, oj1) of one sample as the augmentation maps it into the sample's crop:
//   out[oi][oj] = src[si][sj]: (aa, bb) = transposed ? (oj, oi) : (oi, oj), si = fa ? P - 1 - aa : aa, sj = fb ? P - 1 - bb : bb
//   (util_image.data_aug_np: flag 2 = np.rot90, counter-clockwise; odd flags add flipud)
struct TileSrc {
  long long base, pitch;                         // pool byte offset of the source rectangle's first pixel; bytes per image row
  int si0, sj0, th, tw;                          // the source rectangle within the crop: origin, rows, columns
  bool tr, fa, fb;
};

__device__ __forceinline__ TileSrc tile_source(const PatchArgs& a, int n, int oi0, int oi1, int oj0, int oj1) {
  const int N = a.n, P = a.p;
  const int* const pi = reinterpret_cast<const int*>(a.params);
  const int img = pi[n], y0 = pi[N + n], x0 = pi[2 * N + n], flag = pi[3 * N + n] & 7;
  const long long off = a.table[3 * img], W = a.table[3 * img + 2];
  TileSrc s;
  s.tr = (flag >> 1) & 1; s.fa = (0xD2 >> flag) & 1; s.fb = (0xB4 >> flag) & 1;
  const int a0 = s.tr ? oj0 : oi0, a1 = s.tr ? oj1 : oi1, b0 = s.tr ? oi0 : oj0, b1 = s.tr ? oi1 : oj1;
  s.si0 = s.fa ? P - a1 : a0; s.th = a1 - a0; s.sj0 = s.fb ? P - b1 : b0; s.tw = b1 - b0;
  s.pitch = W * 3;
  s.base = off + ((long long)(y0 + s.si0) * W + (x0 + s.sj0)) * 3;
  return s;
}

// the rectangle's pool bytes -> LDS rows of kRowBytes, by byte loads along source rows; nothing outside the crop is read
template <int POOLS>
__device__ __forceinline__ void stage_tile(const PatchArgs& a, const TileSrc& s, unsigned char* sa, unsigned char* sb, int tid) {
  const int rowb = s.tw * 3;
  for (int idx = tid; idx < s.th * rowb; idx += kThreads) {
    const int r = idx / rowb, k = idx - r * rowb;
    const long long g = s.base + (long long)r * s.pitch + k;
    sa[r * kRowBytes + k] = a.pool_a[g];
    if (POOLS == 2) sb[r * kRowBytes + k] = a.pool_b[g];
  }
}

// the source pixel (si, sj) within the crop of output pixel (oi, oj)
__device__ __forceinline__ void source_pixel(const TileSrc& s, int P, int oi, int oj, int& si, int& sj) {
  const int aa = s.tr ? oj : oi, bb = s.tr ? oi : oj;
  si = s.fa ? P - 1 - aa : aa;
  sj = s.fb ? P - 1 - bb : bb;
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void datagen_patch_kernel(const PatchArgs a) {
  __shared__ unsigned char sb[MODE == kPair ? 2 : 1][kTile * kRowBytes];
  __shared__ float sn[MODE == kDenoise ? 3 * kTile * kNoiseRow : 1];
  __shared__ double se[2];
  const int tid = threadIdx.x;
  const int n = blockIdx.y, N = a.n, P = a.p;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int* const pi = reinterpret_cast<const int*>(a.params);
  const double* const pd = reinterpret_cast<const double*>(a.params + (size_t)32 * N);
  const int oi0 = ty * kTile, oi1 = min(oi0 + kTile, P), oj0 = tx * kTile, oj1 = min(oj0 + kTile, P);
  const TileSrc s = tile_source(a, n, oi0, oi1, oj0, oj1);
  const int si0 = s.si0, th = s.th, sj0 = s.sj0, tw = s.tw;      // the tile's source rectangle

  stage_tile<MODE == kPair ? 2 : 1>(a, s, sb[0], sb[MODE == kPair ? 1 : 0], tid);
  double c_h = 0.0, c_w = 0.0, denom = 1.0, down = 0.0, up = 0.0;
  bool niid = false;
  if (MODE == kDenoise) {
    if (a.noise) {
      const int plane = th * tw;
      for (int idx = tid; idx < 3 * plane; idx += kThreads) {
        const int c = idx / plane, rem = idx - c * plane, r = rem / tw, k = rem - r * tw;
        sn[(c * kTile + r) * kNoiseRow + k] = a.noise[(((long long)n * 3 + c) * P + (si0 + r)) * P + (sj0 + k)];
      }
    } else {
      const long long sid = a.sample_ids[n];
      for (int idx = tid; idx < 3 * th * kQuads; idx += kThreads) {
        const int row = idx / kQuads, qi = idx - row * kQuads, c = row / th, r = row - c * th;
        const unsigned e0 = (unsigned)((c * P + si0 + r) * P + sj0);
        const unsigned q = (e0 >> 2) + (unsigned)qi;
        if (q > ((e0 + (unsigned)tw - 1u) >> 2)) continue;
        float z[4];
        normals4(q, a.stream_id, sid, a.seed, z);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int k = (int)(q * 4u + (unsigned)t) - (int)e0;
          if (k >= 0 && k < tw) sn[(c * kTile + r) * kNoiseRow + k] = z[t];
        }
      }
    }
    niid = pi[4 * N + n] != 0;
    c_h = pd[n]; c_w = pd[N + n]; denom = pd[2 * N + n]; down = pd[3 * N + n]; up = pd[4 * N + n];
    if (niid && tid == 0) {
      // the bump is largest at the pixel nearest the centre and smallest at the corner farthest from it
      const double last = (double)(P - 1);
      const double ih = fmin(floor(c_h), last), iw = fmin(floor(c_w), last);
      const double nh = fmin((ih - c_h) * (ih - c_h), (fmin(ih + 1.0, last) - c_h) * (fmin(ih + 1.0, last) - c_h));
      const double nw = fmin((iw - c_w) * (iw - c_w), (fmin(iw + 1.0, last) - c_w) * (fmin(iw + 1.0, last) - c_w));
      const double fh = fmax((0.0 - c_h) * (0.0 - c_h), (last - c_h) * (last - c_h));
      const double fw = fmax((0.0 - c_w) * (0.0 - c_w), (last - c_w) * (last - c_w));
      se[0] = bump(fh, fw, denom);
      se[1] = bump(nh, nw, denom);
    }
  }
  __syncthreads();

  const int r = tid >> 3, oi = oi0 + r, ojb = oj0 + (tid & 7) * 4;
  if (oi >= oi1 || ojb >= oj1) return;
  const int cnt = min(4, oj1 - ojb);
  const bool vec = a.vec != 0;                   // (the patch size is a multiple of four then, so cnt is 4)
  const double e_min = MODE == kDenoise ? se[0] : 0.0, e_max = MODE == kDenoise ? se[1] : 1.0;
  float v0[3][4], v1[3][4], sg[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int oj = min(ojb + t, oj1 - 1);        // (lanes past the edge repeat the last pixel; their values are not stored)
    int si, sj;
    source_pixel(s, P, oi, oj, si, sj);
    const int lr = si - si0, lk = sj - sj0;
    float sig = 0.f;
    if (MODE == kDenoise) {
      double s64 = down;
      if (niid) {
        const double di = (double)si - c_h, dj = (double)sj - c_w;
        const double e = bump(di * di, dj * dj, denom);
        s64 = down + (e - e_min) / (e_max - e_min) * (up - down);
      }
      sig = (float)s64;
      const float sq = sig * sig;
      sg[t] = sq < 1e-10f ? 1e-10f : sq;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float b = (float)sb[0][lr * kRowBytes + lk * 3 + c];
      if (MODE == kHr) {
        v0[c][t] = b / 255.f;
      } else if (MODE == kPair) {
        v0[c][t] = b * (1.f / 255.f);
        v1[c][t] = (float)sb[MODE == kPair ? 1 : 0][lr * kRowBytes + lk * 3 + c] * (1.f / 255.f);
      } else {
        const float gt = b * (1.f / 255.f);
        const float nz = sn[(c * kTile + lr) * kNoiseRow + lk] * sig;
        float y = gt + nz;
        if (a.clip) y = fminf(fmaxf(y, 0.f), 1.f);
        v0[c][t] = y;
        v1[c][t] = gt;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const size_t o = (((size_t)n * 3 + c) * P + oi) * P + ojb;
    store4(a.out0 + o, cnt, vec, v0[c]);
    if (MODE != kHr) store4(a.out1 + o, cnt, vec, v1[c]);
  }
  if (MODE == kDenoise) store4(a.out2 + ((size_t)n * P + oi) * P + ojb, cnt, vec, sg);
}

// lam x + (1 - lam) y as datasets/data_tools.py:27-28 evaluates it: l1 = 1 - lam, the two products and the sum each round to fp32
__device__ __forceinline__ float mix2(float lam, float l1, float x, float y) {
  const float u = lam * x, v = l1 * y;
  return u + v;
}

__global__ __launch_bounds__(kThreads) void datagen_pair_mix_kernel(const PatchArgs a) {
  __shared__ unsigned char sb[4][kTile * kRowBytes];      // the sample's tile from pool a, pool b; its partner's from pool a, pool b
  const int tid = threadIdx.x;
  const int n = blockIdx.y, N = a.n, P = a.p;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int m = reinterpret_cast<const int*>(a.mix)[n];
  const float lam = reinterpret_cast<const float*>(a.mix + (size_t)4 * N)[n], l1 = 1.f - lam;
  const int oi0 = ty * kTile, oi1 = min(oi0 + kTile, P), oj0 = tx * kTile, oj1 = min(oj0 + kTile, P);
  const TileSrc s = tile_source(a, n, oi0, oi1, oj0, oj1), q = tile_source(a, m, oi0, oi1, oj0, oj1);
  stage_tile<2>(a, s, sb[0], sb[1], tid);
  stage_tile<2>(a, q, sb[2], sb[3], tid);
  __syncthreads();

  const int r = tid >> 3, oi = oi0 + r, ojb = oj0 + (tid & 7) * 4;
  if (oi >= oi1 || ojb >= oj1) return;
  const int cnt = min(4, oj1 - ojb);
  const bool vec = a.vec != 0;                   // (the patch size is a multiple of four then, so cnt is 4)
  float v0[3][4], v1[3][4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int oj = min(ojb + t, oj1 - 1);        // (lanes past the edge repeat the last pixel; their values are not stored)
    int si, sj, qi, qj;
    source_pixel(s, P, oi, oj, si, sj);
    source_pixel(q, P, oi, oj, qi, qj);
    const int is = (si - s.si0) * kRowBytes + (sj - s.sj0) * 3, iq = (qi - q.si0) * kRowBytes + (qj - q.sj0) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v0[c][t] = mix2(lam, l1, (float)sb[0][is + c] * (1.f / 255.f), (float)sb[2][iq + c] * (1.f / 255.f));
      v1[c][t] = mix2(lam, l1, (float)sb[1][is + c] * (1.f / 255.f), (float)sb[3][iq + c] * (1.f / 255.f));
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const size_t o = (((size_t)n * 3 + c) * P + oi) * P + ojb;
    store4(a.out0 + o, cnt, vec, v0[c]);
    store4(a.out1 + o, cnt, vec, v1[c]);
  }
}

__device__ __forceinline__ void load4(const float* q, int cnt, bool vec, float (&r)[4]) {
  if (vec) {
    const float4 v = *reinterpret_cast<const float4*>(q);
    r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = k < cnt ? q[k] : 0.f;
  }
}

__global__ __launch_bounds__(kThreads) void mixup_kernel(const float* a, const float* b, const unsigned char* mix, float* out_a, float* out_b, int N,
                                                         long long per, int vec) {
  const long long e = ((long long)blockIdx.x * kThreads + threadIdx.x) * 4;
  if (e >= per) return;
  const int n = blockIdx.y;
  const int m = reinterpret_cast<const int*>(mix)[n];
  const float lam = reinterpret_cast<const float*>(mix + (size_t)4 * N)[n], l1 = 1.f - lam;
  const int cnt = per - e < 4 ? (int)(per - e) : 4;
  const size_t own = (size_t)n * per + e, other = (size_t)m * per + e;
  float x[4], y[4], r[4];
  load4(a + own, cnt, vec != 0, x);
  load4(a + other, cnt, vec != 0, y);
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = mix2(lam, l1, x[k], y[k]);
  store4(out_a + own, cnt, vec != 0, r);
  load4(b + own, cnt, vec != 0, x);
  load4(b + other, cnt, vec != 0, y);
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = mix2(lam, l1, x[k], y[k]);
  store4(out_b + own, cnt, vec != 0, r);
}

__global__ __launch_bounds__(kThreads) void datagen_normal_kernel(float* out, long long per, const long long* sample_ids, unsigned long long seed,
                                                                  unsigned stream_id, int vec) {
  const long long q = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long e = q * 4;
  if (e >= per) return;
  const int n = blockIdx.y;
  float z[4];
  normals4((unsigned)q, stream_id, sample_ids[n], seed, z);
  const int cnt = per - e < 4 ? (int)(per - e) : 4;
  store4(out + (size_t)n * per + e, cnt, vec != 0, z);
}

// fixed-order reductions over the block (lanes by shuffle tree, then waves 0..3); the result is valid in every thread
__device__ __forceinline__ double block_max(double v, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  __syncthreads();
  return m;
}

__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return s;
}

constexpr int kBlurPerThread = (VIRNET_DATAGEN_MAX_KERNEL * VIRNET_DATAGEN_MAX_KERNEL + kThreads - 1) / kThreads;

__global__ __launch_bounds__(kThreads) void datagen_blur_kernel(const double* lam1_sq, const double* lam2_sq, const double* theta, int k, float center,
                                                                float* kernel, float* kinfo) {
  __shared__ double red[kThreads / 64];
  const int n = blockIdx.x, tid = threadIdx.x;
  const double l1 = lam1_sq[n], l2 = lam2_sq[n];
  double s, c;
  sincos(theta[n], &s, &c);
  // sigma = U diag(l1, l2) U^T with U = [[c, -s], [s, c]]
  const double u00 = c * l1, u01 = -s * l2, u10 = s * l1, u11 = c * l2;
  const double s00 = u00 * c + u01 * -s, s01 = u00 * s + u01 * c, s10 = u10 * c + u11 * -s, s11 = u10 * s + u11 * c;
  const double det = s00 * s11 - s01 * s10;
  const double p00 = s11 / det, p01 = -s01 / det, p10 = -s10 / det, p11 = s00 / det;
  double q[kBlurPerThread];
  double m = -INFINITY;
#pragma unroll
  for (int j = 0; j < kBlurPerThread; ++j) {
    const int idx = tid + j * kThreads;
    q[j] = -INFINITY;
    if (idx < k * k) {
      const int row = idx / k, col = idx - row * k;
      // (the reference builds its grid in fp32: a half-pixel centre stays exact)
      const double dx = (double)((float)col - center), dy = (double)((float)row - center);
      q[j] = -0.5 * (p00 * dx * dx + (p01 + p10) * dx * dy + p11 * dy * dy);
    }
    m = fmax(m, q[j]);
  }
  m = block_max(m, red);
  double e[kBlurPerThread], sum = 0.0;
#pragma unroll
  for (int j = 0; j < kBlurPerThread; ++j) {
    e[j] = tid + j * kThreads < k * k ? exp(q[j] - m) : 0.0;
    sum += e[j];
  }
  sum = block_sum(sum, red);
#pragma unroll
  for (int j = 0; j < kBlurPerThread; ++j) {
    const int idx = tid + j * kThreads;
    if (idx < k * k) kernel[(size_t)n * k * k + idx] = (float)(e[j] / sum);
  }
  if (tid == 0) {
    kinfo[3 * n] = (float)s00;
    kinfo[3 * n + 1] = (float)s11;
    kinfo[3 * n + 2] = (float)(s01 / (sqrt(s00) * sqrt(s11)));
  }
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// [p, p + pb) and [q, q + qb) share no byte
bool disjoint(const void* p, unsigned long long pb, const void* q, unsigned long long qb) {
  const unsigned long long x = (unsigned long long)(uintptr_t)p, y = (unsigned long long)(uintptr_t)q;
  return x + pb <= y || y + qb <= x;
}

}  // namespace

extern "C" int virnet_datagen_patches(int mode, const void* pool_a, const void* pool_b, const long long* table, const void* params, int n, int p,
                                      const float* noise, const long long* sample_ids, unsigned long long seed, int stream_id, int clip,
                                      float* out0, float* out1, float* out2, void* stream) {
  const char* const who = "virnet_datagen_patches";
  VIRNET_REQUIRE(mode >= VIRNET_DATAGEN_DENOISE && mode <= VIRNET_DATAGEN_HR, "%s: mode %d (0 denoise, 1 pair, 2 hr expected)", who, mode);
  VIRNET_REQUIRE(n >= 1 && n <= 65535, "%s: %d samples (1 .. 65535 expected)", who, n);
  VIRNET_REQUIRE(p >= 1 && p <= VIRNET_DATAGEN_MAX_PATCH, "%s: patch size %d (1 .. %d expected)", who, p, VIRNET_DATAGEN_MAX_PATCH);
  VIRNET_REQUIRE(pool_a && table && params && out0, "%s: NULL pointer", who);
  VIRNET_REQUIRE(aligned(table, 8) && aligned(params, 8), "%s: table and params must be 8-byte aligned", who);
  VIRNET_REQUIRE(mode == VIRNET_DATAGEN_HR || out1, "%s: NULL second output", who);
  VIRNET_REQUIRE(mode != VIRNET_DATAGEN_PAIR || pool_b, "%s: the pair mode takes two pools", who);
  VIRNET_REQUIRE(mode != VIRNET_DATAGEN_DENOISE || (out2 && (noise || sample_ids)), "%s: the denoise mode takes a third output and noise or sample ids", who);
  VIRNET_REQUIRE(aligned(out0, 4) && aligned(out1, 4) && aligned(out2, 4) && aligned(noise, 4) && aligned(sample_ids, 8), "%s: misaligned pointer", who);
  PatchArgs a{};
  a.pool_a = static_cast<const unsigned char*>(pool_a);
  a.pool_b = static_cast<const unsigned char*>(pool_b);
  a.table = table;
  a.params = static_cast<const unsigned char*>(params);
  a.noise = noise;
  a.sample_ids = sample_ids;
  a.out0 = out0; a.out1 = out1; a.out2 = out2;
  a.seed = seed;
  a.stream_id = (unsigned)stream_id;
  a.n = n; a.p = p;
  a.tiles_x = (p + kTile - 1) / kTile;
  a.clip = clip != 0;
  a.vec = p % 4 == 0 && aligned(out0, 16) && aligned(out1, 16) && aligned(out2, 16);
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_x), (unsigned)n);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mode == VIRNET_DATAGEN_DENOISE)
    hipLaunchKernelGGL((datagen_patch_kernel<kDenoise>), grid, dim3(kThreads), 0, s, a);
  else if (mode == VIRNET_DATAGEN_PAIR)
    hipLaunchKernelGGL((datagen_patch_kernel<kPair>), grid, dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL((datagen_patch_kernel<kHr>), grid, dim3(kThreads), 0, s, a);
  return virnet::check_launch("datagen patch launch");
}

extern "C" int virnet_datagen_normal(float* out, int n, long long per, const long long* sample_ids, unsigned long long seed, int stream_id,
                                     void* stream) {
  const char* const who = "virnet_datagen_normal";
  VIRNET_REQUIRE(n >= 1 && n <= 65535, "%s: %d samples (1 .. 65535 expected)", who, n);
  VIRNET_REQUIRE(per >= 1 && per < (1ll << 31), "%s: %lld elements per sample (1 .. 2^31 - 1 expected)", who, per);
  VIRNET_REQUIRE(out && sample_ids && aligned(out, 4) && aligned(sample_ids, 8), "%s: NULL or misaligned pointer", who);
  const long long quads = (per + 3) / 4;
  const dim3 grid((unsigned)((quads + kThreads - 1) / kThreads), (unsigned)n);
  hipLaunchKernelGGL(datagen_normal_kernel, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), out, per, sample_ids, seed,
                     (unsigned)stream_id, (int)(per % 4 == 0 && aligned(out, 16)));
  return virnet::check_launch("datagen normal launch");
}

extern "C" int virnet_datagen_blur_kernels(const double* lam1_sq, const double* lam2_sq, const double* theta, int n, int k, int sf, int shift,
                                           float* kernel, float* kinfo, void* stream) {
  const char* const who = "virnet_datagen_blur_kernels";
  VIRNET_REQUIRE(n >= 1, "%s: %d samples (at least 1 expected)", who, n);
  VIRNET_REQUIRE(k >= 1 && k <= VIRNET_DATAGEN_MAX_KERNEL && k % 2 == 1, "%s: kernel size %d (odd, 1 .. %d expected)", who, k, VIRNET_DATAGEN_MAX_KERNEL);
  VIRNET_REQUIRE(sf >= 1 && sf <= 4, "%s: scale factor %d (1 .. 4 expected)", who, sf);
  VIRNET_REQUIRE(lam1_sq && lam2_sq && theta && kernel && kinfo, "%s: NULL pointer", who);
  VIRNET_REQUIRE(aligned(lam1_sq, 8) && aligned(lam2_sq, 8) && aligned(theta, 8) && aligned(kernel, 4) && aligned(kinfo, 4), "%s: misaligned pointer", who);
  const float center = (float)(k / 2) + (shift ? 0.5f * (float)(sf - k % 2) : 0.f);
  hipLaunchKernelGGL(datagen_blur_kernel, dim3((unsigned)n), dim3(kThreads), 0, static_cast<hipStream_t>(stream), lam1_sq, lam2_sq, theta, k, center,
                     kernel, kinfo);
  return virnet::check_launch("datagen blur-kernel launch");
}

extern "C" int virnet_mixup(const float* a, const float* b, const void* mix, float* out_a, float* out_b, int n, long long per, void* stream) {
  const char* const who = "virnet_mixup";
  VIRNET_REQUIRE(n >= 1 && n <= 65535, "%s: %d samples (1 .. 65535 expected)", who, n);
  VIRNET_REQUIRE(per >= 1 && per < (1ll << 31), "%s: %lld elements per sample (1 .. 2^31 - 1 expected)", who, per);
  VIRNET_REQUIRE(a && b && mix && out_a && out_b, "%s: NULL pointer", who);
  VIRNET_REQUIRE(aligned(a, 4) && aligned(b, 4) && aligned(mix, 4) && aligned(out_a, 4) && aligned(out_b, 4), "%s: misaligned pointer", who);
  const unsigned long long bytes = (unsigned long long)n * (unsigned long long)per * 4ull, mix_bytes = 8ull * (unsigned long long)n;
  VIRNET_REQUIRE(disjoint(out_a, bytes, out_b, bytes), "%s: the outputs overlap each other", who);
  for (float* const out : {out_a, out_b})
    VIRNET_REQUIRE(disjoint(out, bytes, a, bytes) && disjoint(out, bytes, b, bytes) && disjoint(out, bytes, mix, mix_bytes),
                   "%s: an output overlaps an input (samples are gathered through perm: the mix cannot run in place)", who);
  const long long quads = (per + 3) / 4;
  const dim3 grid((unsigned)((quads + kThreads - 1) / kThreads), (unsigned)n);
  const int vec = per % 4 == 0 && aligned(a, 16) && aligned(b, 16) && aligned(out_a, 16) && aligned(out_b, 16);
  hipLaunchKernelGGL(mixup_kernel, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), a, b, static_cast<const unsigned char*>(mix), out_a,
                     out_b, n, per, vec);
  return virnet::check_launch("mixup launch");
}

extern "C" int virnet_datagen_pair_mix(const void* pool_a, const void* pool_b, const long long* table, const void* params, const void* mix, int n,
                                       int p, float* out0, float* out1, void* stream) {
  const char* const who = "virnet_datagen_pair_mix";
  VIRNET_REQUIRE(n >= 1 && n <= 65535, "%s: %d samples (1 .. 65535 expected)", who, n);
  VIRNET_REQUIRE(p >= 1 && p <= VIRNET_DATAGEN_MAX_PATCH, "%s: patch size %d (1 .. %d expected)", who, p, VIRNET_DATAGEN_MAX_PATCH);
  VIRNET_REQUIRE(pool_a && pool_b && table && params && mix && out0 && out1, "%s: NULL pointer", who);
  VIRNET_REQUIRE(aligned(table, 8) && aligned(params, 8), "%s: table and params must be 8-byte aligned", who);
  VIRNET_REQUIRE(aligned(mix, 4) && aligned(out0, 4) && aligned(out1, 4), "%s: misaligned pointer", who);
  const unsigned long long bytes = (unsigned long long)n * 3ull * (unsigned long long)p * (unsigned long long)p * 4ull;
  VIRNET_REQUIRE(disjoint(out0, bytes, out1, bytes), "%s: the outputs overlap each other", who);
  for (float* const out : {out0, out1})
    VIRNET_REQUIRE(disjoint(out, bytes, params, 96ull * (unsigned long long)n) && disjoint(out, bytes, mix, 8ull * (unsigned long long)n) &&
                       disjoint(out, bytes, pool_a, 1) && disjoint(out, bytes, pool_b, 1) && disjoint(out, bytes, table, 1),
                   "%s: an output overlaps an input", who);
  PatchArgs a{};
  a.pool_a = static_cast<const unsigned char*>(pool_a);
  a.pool_b = static_cast<const unsigned char*>(pool_b);
  a.table = table;
  a.params = static_cast<const unsigned char*>(params);
  a.mix = static_cast<const unsigned char*>(mix);
  a.out0 = out0; a.out1 = out1;
  a.n = n; a.p = p;
  a.tiles_x = (p + kTile - 1) / kTile;
  a.vec = p % 4 == 0 && aligned(out0, 16) && aligned(out1, 16);
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_x), (unsigned)n);
  hipLaunchKernelGGL(datagen_pair_mix_kernel, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return virnet::check_launch("datagen pair-mix launch");
}

// ---- the validation set of the denoising training (SimulateTest, datasets/DenoisingDatasets.py:255-296) -------------------------------------
//   simulate_test_kernel         one thread per pixel of one image: its three pool bytes -> gt = u8 / 255 as a true fp32 division
//                                (util_image.imread, utils/util_image.py:206), the three normals noise[y][x][0..2] of the ONE noise array
//                                of the whole set (row stride w_max, not w), sigma[ys[y]][xs[x]] of the 256 x 256 map (the nearest-exact
//                                source indices come from the host), noisy = gt + fp32(noise * sigma); three coalesced stores per output.
namespace {

constexpr int kSimMap = VIRNET_SIMTEST_MAP;

__global__ __launch_bounds__(kThreads) void simulate_test_kernel(const unsigned char* pool, const long long* table, const int* indices,
                                                                 const float* noise, const float* sigma, const int* ys, const int* xs, int h,
                                                                 int w, int w_max, float* im_noisy, float* im_gt) {
  const long long pix = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long plane = (long long)h * w;
  if (pix >= plane) return;
  const int n = blockIdx.y;
  const int y = (int)(pix / w), x = (int)(pix - (long long)y * w);
  const unsigned char* src = pool + table[(size_t)indices[n] * 3] + pix * 3;
  const float* nz = noise + ((size_t)y * w_max + x) * 3;
  const float s = sigma[ys[y] * kSimMap + xs[x]];
  const size_t o = (size_t)n * 3 * plane + pix;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float gt = (float)src[c] / 255.f;
    const float prod = nz[c] * s;
    im_gt[o + c * plane] = gt;
    im_noisy[o + c * plane] = gt + prod;
  }
}

}  // namespace

extern "C" int virnet_datagen_simulate_test(const void* pool, const long long* table, const int* indices, const float* noise, const float* sigma,
                                            const int* ys, const int* xs, int n, int h, int w, int h_max, int w_max, float* im_noisy,
                                            float* im_gt, void* stream) {
  const char* const who = "virnet_datagen_simulate_test";
  VIRNET_REQUIRE(n >= 1 && n <= 65535, "%s: %d images (1 .. 65535 expected)", who, n);
  VIRNET_REQUIRE(h >= 1 && w >= 1 && h <= h_max && w <= w_max, "%s: image %d x %d outside the noise array %d x %d", who, h, w, h_max, w_max);
  VIRNET_REQUIRE((long long)h * w < (1ll << 31) / 3, "%s: image %d x %d: fewer than 2^31 / 3 pixels expected", who, h, w);
  VIRNET_REQUIRE(pool && table && indices && noise && sigma && ys && xs && im_noisy && im_gt, "%s: NULL pointer", who);
  VIRNET_REQUIRE(aligned(table, 8), "%s: table must be 8-byte aligned", who);
  VIRNET_REQUIRE(aligned(indices, 4) && aligned(noise, 4) && aligned(sigma, 4) && aligned(ys, 4) && aligned(xs, 4) && aligned(im_noisy, 4) &&
                     aligned(im_gt, 4), "%s: misaligned pointer", who);
  const unsigned long long bytes = (unsigned long long)n * 3ull * (unsigned long long)h * (unsigned long long)w * 4ull;
  VIRNET_REQUIRE(disjoint(im_noisy, bytes, im_gt, bytes), "%s: the outputs overlap each other", who);
  for (float* const out : {im_noisy, im_gt})
    VIRNET_REQUIRE(disjoint(out, bytes, noise, (unsigned long long)h_max * (unsigned long long)w_max * 12ull) &&
                       disjoint(out, bytes, sigma, (unsigned long long)kSimMap * kSimMap * 4ull) && disjoint(out, bytes, indices, 4ull * n) &&
                       disjoint(out, bytes, ys, 4ull * h) && disjoint(out, bytes, xs, 4ull * w) && disjoint(out, bytes, pool, 1) &&
                       disjoint(out, bytes, table, 1),
                   "%s: an output overlaps an input", who);
  const long long plane = (long long)h * w;
  const dim3 grid((unsigned)((plane + kThreads - 1) / kThreads), (unsigned)n);
  hipLaunchKernelGGL(simulate_test_kernel, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), static_cast<const unsigned char*>(pool),
                     table, indices, noise, sigma, ys, xs, h, w, w_max, im_noisy, im_gt);
  return virnet::check_launch("datagen simulate-test launch");
}
