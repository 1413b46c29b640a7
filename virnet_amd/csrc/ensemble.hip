// ensemble.hip -- the 8-way flip / rotation self-ensemble of the real-noise evaluation on the device (host definition:
// virnet_amd/ensemble.py on eval.dihedral / dihedral_inverse; reference: scripts/denoising_virnet_real_sidd.py:113-154,
// dnd_submission_py/pytorch_wrapper.py:15-47, utils/util_image.py:391-466).
//
// Orientation m of an H x W image S is D_m (m // 2 quarter turns counter-clockwise, then an up-down flip for odd m):
//   m = 0, 1, 4, 5 (H x W):  D[i][j] = S[fy ? H-1-i : i][fx ? W-1-j : j]     (fy, fx) = (0,0) (1,0) (1,1) (0,1)
//   m = 2, 3, 6, 7 (W x H):  D[i][j] = S[fy ? H-1-j : j][fx ? W-1-i : i]     (fy, fx) = (0,1) (0,0) (1,0) (1,1)
// so there are two destination groups, even = [4B][C][H][W] and odd = [4B][C][W][H], image b*4 + p with p the position of m in
// (0,1,4,5) / (2,3,6,7).
//
//   ensemble_expand_kernel<SRC>         one workgroup per 32 x 32 source tile per image: the tile (HWC, uint8 or fp32) goes to LDS ONCE as
//                                       fp32 planes and all eight orientations are written from it.  The four keeping modes read LDS
//                                       rows, the four transposing modes read LDS columns (row pitch 33 words: no bank conflict), so a
//                                       half-wave always writes one contiguous run along the destination's x.  uint8 -> fp32 is the
//                                       correctly rounded quotient u / 255 (np.float32(u / 255.0)); fp32 passes through bit for bit.
//   ensemble_reduce_kernel<DST, ORDER>  the inverse, one workgroup per 32 x 32 OUTPUT tile per image: the four keeping modes are read
//                                       straight from global memory (contiguous along x), the four transposing modes are read along
//                                       THEIR x into LDS and taken out transposed.  The eight values of a pixel are added in fp32 in the
//                                       order of the host expression (sequential: the SIDD script's +=; pairwise: numpy's mean over a
//                                       contiguous axis of eight), scaled by 1/8 (exact), clipped and optionally quantised
//                                       (quantize.h: the arithmetic of virnet_quantize_u8).  An HWC result is put together in LDS and
//                                       written as whole pixel rows.  modes == 1: orientation 0 only (no sum, no scaling).
//
// Edge tiles are predicated.  No atomics, no scratch, no synchronisation; every output element is a function of its own pixel's inputs
// only, so the results are bitwise reproducible and independent of the batch an image sits in.
#include "common.h"
#include "quantize.h"
#include "../../include/virnet_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;
constexpr int kPitch = kTile + 1;          // words per LDS row: a column read touches 32 different banks
constexpr int kMaxC = 3;
constexpr int kRows = kThreads / kTile;    // 8 tile rows per pass
constexpr int kOutPitch = kTile * kMaxC + 1;

enum Order { kSequential = 0, kPairwise = 1 };

// (fy, fx) of the keeping modes (0,1,4,5) and of the transposing modes (2,3,6,7), by position in the group
__device__ __forceinline__ bool keep_fy(int p) { return p == 1 || p == 2; }
__device__ __forceinline__ bool keep_fx(int p) { return p >= 2; }
__device__ __forceinline__ bool turn_fy(int p) { return p >= 2; }
__device__ __forceinline__ bool turn_fx(int p) { return p == 0 || p == 3; }

struct ExpandArgs {
  const void* src;     // [b][h][w][c]
  float* even;         // [4b][c][h][w]   (modes == 1: [b][c][h][w])
  float* odd;          // [4b][c][w][h]
  int h, w, c, tiles_x, modes;
};

template <typename SRC>
__device__ __forceinline__ float to_unit(SRC v);
template <>
__device__ __forceinline__ float to_unit<unsigned char>(unsigned char v) { return (float)v / 255.f; }     // IEEE division
template <>
__device__ __forceinline__ float to_unit<float>(float v) { return v; }

template <typename SRC>
__global__ __launch_bounds__(kThreads) void ensemble_expand_kernel(const ExpandArgs k) {
  __shared__ float tile[kMaxC][kTile][kPitch];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int ty = blockIdx.x / k.tiles_x, tx = blockIdx.x - ty * k.tiles_x;
  const int y0 = ty * kTile, x0 = tx * kTile;
  const int H = k.h, W = k.w, C = k.c;
  const int hv = min(kTile, H - y0), wv = min(kTile, W - x0);          // valid extent of this tile

  // ---- stage: a tile row is wv * C contiguous source elements
  const SRC* const src = static_cast<const SRC*>(k.src) + ((size_t)b * H + y0) * W * C + (size_t)x0 * C;
  const int run = kTile * C;
  for (int i = tid; i < kTile * run; i += kThreads) {
    const int ly = i / run, r = i - ly * run;
    const int lx = r / C, ch = r - lx * C;
    if (ly < hv && lx < wv) tile[ch][ly][lx] = to_unit<SRC>(src[(size_t)ly * W * C + r]);
  }
  __syncthreads();

  const int l = tid & (kTile - 1), r0 = tid >> 5;
  const size_t plane = (size_t)H * W;
  const int img_step = k.modes == 8 ? 4 : 1;
  for (int ch = 0; ch < C; ++ch) {
#pragma unroll
    for (int pass = 0; pass < kTile / kRows; ++pass) {
      const int r = r0 + pass * kRows;
      // keeping modes: lane = source x, row = source y
      if (r < hv && l < wv) {
        const float v = tile[ch][r][l];
        const int sy = y0 + r, sx = x0 + l;
        for (int p = 0; p < (k.modes == 8 ? 4 : 1); ++p) {
          const int i = keep_fy(p) ? H - 1 - sy : sy, j = keep_fx(p) ? W - 1 - sx : sx;
          k.even[(((size_t)b * img_step + p) * C + ch) * plane + (size_t)i * W + j] = v;
        }
      }
      // transposing modes: lane = source y (the destination's x), row = source x
      if (k.modes == 8 && l < hv && r < wv) {
        const float v = tile[ch][l][r];
        const int sy = y0 + l, sx = x0 + r;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int i = turn_fx(p) ? W - 1 - sx : sx, j = turn_fy(p) ? H - 1 - sy : sy;
          k.odd[(((size_t)b * 4 + p) * C + ch) * plane + (size_t)i * H + j] = v;
        }
      }
    }
  }
}

struct ReduceArgs {
  const float* even;   // [4b][c][h][w]   (modes == 1: [b][c][h][w])
  const float* odd;    // [4b][c][w][h]
  void* dst;           // [b][h][w][c] or [b][c][h][w]
  int h, w, c, tiles_x, modes, chw;
};

template <typename DST>
__device__ __forceinline__ DST finish(float v);
template <>
__device__ __forceinline__ unsigned char finish<unsigned char>(float v) { return (unsigned char)virnet::quant_u8(v); }
template <>
__device__ __forceinline__ float finish<float>(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }   // np.clip: -0 and NaN pass

template <typename DST, int ORDER>
__global__ __launch_bounds__(kThreads) void ensemble_reduce_kernel(const ReduceArgs k) {
  __shared__ float turned[4][kTile][kPitch];        // the transposing modes' values, [output y][output x]
  __shared__ DST rows[kTile][kOutPitch];            // an HWC result tile, [y][x * C + ch]
  const int tid = threadIdx.x, b = blockIdx.y;
  const int ty = blockIdx.x / k.tiles_x, tx = blockIdx.x - ty * k.tiles_x;
  const int y0 = ty * kTile, x0 = tx * kTile;
  const int H = k.h, W = k.w, C = k.c;
  const int hv = min(kTile, H - y0), wv = min(kTile, W - x0);
  const int l = tid & (kTile - 1), r0 = tid >> 5;
  const size_t plane = (size_t)H * W;
  const bool flip = k.modes == 8;
  const bool stage_out = !k.chw && C > 1;
  DST* const dst = static_cast<DST*>(k.dst);

  for (int ch = 0; ch < C; ++ch) {
    if (flip) {
      if (ch) __syncthreads();                      // the previous channel's reads of `turned` are done
      // lane = output y (the source's x), row = output x
#pragma unroll
      for (int pass = 0; pass < kTile / kRows; ++pass) {
        const int r = r0 + pass * kRows;
        if (l < hv && r < wv) {
          const int sy = y0 + l, sx = x0 + r;
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const int i = turn_fx(p) ? W - 1 - sx : sx, j = turn_fy(p) ? H - 1 - sy : sy;
            turned[p][l][r] = k.odd[(((size_t)b * 4 + p) * C + ch) * plane + (size_t)i * H + j];
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int pass = 0; pass < kTile / kRows; ++pass) {
      const int r = r0 + pass * kRows;
      if (r < hv && l < wv) {
        const int sy = y0 + r, sx = x0 + l;
        float v;
        if (flip) {
          float kv[4];
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const int i = keep_fy(p) ? H - 1 - sy : sy, j = keep_fx(p) ? W - 1 - sx : sx;
            kv[p] = k.even[(((size_t)b * 4 + p) * C + ch) * plane + (size_t)i * W + j];
          }
          // modes in order: 0 1 | 2 3 | 4 5 | 6 7
          const float m0 = kv[0], m1 = kv[1], m2 = turned[0][r][l], m3 = turned[1][r][l];
          const float m4 = kv[2], m5 = kv[3], m6 = turned[2][r][l], m7 = turned[3][r][l];
          float acc = 0.f;                          // +0: a sum of negative zeros is +0 in both host expressions
          if (ORDER == kSequential) {
            acc += m0; acc += m1; acc += m2; acc += m3; acc += m4; acc += m5; acc += m6; acc += m7;
          } else {
            acc += ((m0 + m1) + (m2 + m3)) + ((m4 + m5) + (m6 + m7));
          }
          v = acc / 8.f;
        } else {
          v = k.even[((size_t)b * C + ch) * plane + (size_t)sy * W + sx];
        }
        const DST o = finish<DST>(v);
        if (stage_out) rows[r][l * C + ch] = o;
        else dst[((size_t)b * C + ch) * plane + (size_t)sy * W + sx] = o;         // (C == 1: HWC is CHW)
      }
    }
  }
  if (stage_out) {
    __syncthreads();
    DST* const out = dst + ((size_t)b * H + y0) * W * C + (size_t)x0 * C;
    const int run = kTile * C, valid = wv * C;
    for (int i = tid; i < kTile * run; i += kThreads) {
      const int ly = i / run, r = i - ly * run;
      if (ly < hv && r < valid) out[(size_t)ly * W * C + r] = rows[ly][r];
    }
  }
}

int geometry(const char* who, int b, int h, int w, int c, int modes, int* tiles_x, long long* tiles) {
  VIRNET_REQUIRE(modes == 1 || modes == 8, "%s: modes %d (1 or 8 expected)", who, modes);
  VIRNET_REQUIRE(c == 1 || c == 3, "%s: %d channels (1 or 3 expected)", who, c);
  VIRNET_REQUIRE(b > 0 && b <= 65535, "%s: batch %d outside 1..65535", who, b);
  VIRNET_REQUIRE(h > 0 && w > 0 && h <= (1 << 20) && w <= (1 << 20), "%s: bad size %dx%d", who, h, w);
  *tiles_x = (w + kTile - 1) / kTile;
  *tiles = (long long)*tiles_x * ((h + kTile - 1) / kTile);
  VIRNET_REQUIRE(*tiles <= (1ll << 30), "%s: %dx%d is too large (%lld tiles)", who, h, w, *tiles);
  return 0;
}

}  // namespace

extern "C" int virnet_ensemble_expand(const void* src, int src_is_f32, float* even, float* odd, int b, int h, int w, int c, int modes,
                                      void* stream) {
  int tiles_x;
  long long tiles;
  if (geometry("virnet_ensemble_expand", b, h, w, c, modes, &tiles_x, &tiles)) return 1;
  VIRNET_REQUIRE(src && even && (odd || modes == 1), "virnet_ensemble_expand: NULL pointer");
  VIRNET_REQUIRE((((uintptr_t)even | (uintptr_t)odd) & 3) == 0 && (!src_is_f32 || ((uintptr_t)src & 3) == 0),
                 "virnet_ensemble_expand: misaligned float32 tensor");
  const ExpandArgs k{src, even, odd, h, w, c, tiles_x, modes};
  const dim3 grid((unsigned)tiles, b);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (src_is_f32) hipLaunchKernelGGL(ensemble_expand_kernel<float>, grid, dim3(kThreads), 0, s, k);
  else hipLaunchKernelGGL(ensemble_expand_kernel<unsigned char>, grid, dim3(kThreads), 0, s, k);
  return virnet::check_launch("ensemble_expand launch");
}

extern "C" int virnet_ensemble_reduce(const float* even, const float* odd, void* dst, int dst_is_f32, int pairwise, int chw, int b, int h, int w,
                                      int c, int modes, void* stream) {
  int tiles_x;
  long long tiles;
  if (geometry("virnet_ensemble_reduce", b, h, w, c, modes, &tiles_x, &tiles)) return 1;
  VIRNET_REQUIRE(even && dst && (odd || modes == 1), "virnet_ensemble_reduce: NULL pointer");
  VIRNET_REQUIRE((((uintptr_t)even | (uintptr_t)odd) & 3) == 0 && (!dst_is_f32 || ((uintptr_t)dst & 3) == 0),
                 "virnet_ensemble_reduce: misaligned float32 tensor");
  const ReduceArgs k{even, odd, dst, h, w, c, tiles_x, modes, chw != 0};
  const dim3 grid((unsigned)tiles, b);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dst_is_f32) {
    if (pairwise) hipLaunchKernelGGL((ensemble_reduce_kernel<float, kPairwise>), grid, dim3(kThreads), 0, s, k);
    else hipLaunchKernelGGL((ensemble_reduce_kernel<float, kSequential>), grid, dim3(kThreads), 0, s, k);
  } else {
    if (pairwise) hipLaunchKernelGGL((ensemble_reduce_kernel<unsigned char, kPairwise>), grid, dim3(kThreads), 0, s, k);
    else hipLaunchKernelGGL((ensemble_reduce_kernel<unsigned char, kSequential>), grid, dim3(kThreads), 0, s, k);
  }
  return virnet::check_launch("ensemble_reduce launch");
}
