// restore.hip -- the two ends of tiled whole-image restoration (host definition: gather_np / blend_np of virnet_amd/restore.py; the grid
// is the one of utils/tiling.forward_tiled).  Between them sits the ordinary forward on a batch of tiles, which never sees more than one
// tile: only these two kernels touch the whole image.
//
//   tile_gather_kernel<SRC>      boxes of a device-resident image (uint8 or fp32; HWC or CHW; 1..4 channels) -> one fp32 NCHW batch.  One
//                                workgroup owns kRows rows x kChunk columns of one box.  A source row segment is one contiguous run (HWC:
//                                cols * C elements of a pixel row; CHW: cols elements of a plane row) and is read along that run: uint8 as
//                                whole aligned dwords with at most three single bytes at either end (only dwords that lie INSIDE the run
//                                are read, whatever the 3-byte pixel stride does to its alignment), fp32 as dwords.  The values are laid
//                                into LDS as fp32 planes [row][channel][x] (uint8 -> the correctly rounded quotient u / 255, fp32 bit for
//                                bit) and leave as rows of the destination planes: 16-byte stores over the 16-byte grid of the destination
//                                row, at most three scalar stores in front of it and behind it (tw % 4 != 0 moves that grid from row to row).
//   tile_blend_kernel<DST,C,CROP> the restored tile stack [ny * nx][C][th][tw] -> one image.  A thread owns four adjacent pixels of one
//                                output row.  The plan's tap tables give, per output row and per output column, up to VIRNET_TILE_SLOTS
//                                (tile index along the axis, fp32 weight) slots in ascending tile order, -1 = unused.  CROP: slot 0 of either
//                                axis names the owner and its value is COPIED.  Otherwise acc = +0; for every used row slot, for every used
//                                column slot: acc = fl(acc + fl(fl(wy * wx) * v)) -- no contraction, unused slots are skipped (not
//                                multiplied by zero), so a NaN stays inside the support of the tile that holds it.  Then the clip and,
//                                for uint8, the quantisation of quantize.h.  Tile bases are 64-bit, indices inside a tile and inside the
//                                output 32-bit.  A slot whose tile index or local coordinate falls outside the stack is skipped: no table
//                                content can make the kernel read outside `tiles`.
//
// Edge workgroups are predicated.  No atomics, no scratch, no inter-workgroup or host synchronisation; every output element is a function
// of its own taps only: bitwise reproducible, capturable, independent of how the boxes are cut into launches.
#include "common.h"
#include "quantize.h"
#include "../../include/virnet_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxC = 4;
constexpr int kRows = 4;                 // box rows per gather workgroup
constexpr int kChunk = 512;              // box columns per gather workgroup
constexpr int kPitch = kChunk + 12;      // words per LDS plane row: 16-byte aligned, and the C planes of one pixel sit 12 banks apart
constexpr int kPx = 4;                   // output pixels per blend thread
constexpr int kSlots = VIRNET_TILE_SLOTS;

struct GatherArgs {
  const void* src;
  float* dst;
  int h, w, c, chw, th, tw, xchunks;
  int box[VIRNET_TILE_BOXES][2];         // (y, x) of each box of this launch
};

__device__ __forceinline__ int div_small(int j, int c) {
  switch (c) {
    case 1: return j;
    case 2: return j >> 1;
    case 3: return j / 3;
    default: return j >> 2;
  }
}

__device__ __forceinline__ float unit_of(unsigned v) { return (float)v / 255.f; }     // IEEE division: np.float32(u / 255.0)

template <typename SRC>
__global__ __launch_bounds__(kThreads) void tile_gather_kernel(const GatherArgs k) {
  __shared__ __attribute__((aligned(16))) float stage[kRows][kMaxC][kPitch];
  const int tid = threadIdx.x, tile = blockIdx.y;
  const int band = blockIdx.x / k.xchunks, xc = blockIdx.x - band * k.xchunks;
  const int r0 = band * kRows, c0 = xc * kChunk;
  const int rows = min(kRows, k.th - r0), cols = min(kChunk, k.tw - c0);
  const int y0 = k.box[tile][0] + r0, x0 = k.box[tile][1] + c0;
  const int C = k.c;
  const int inter = k.chw ? 1 : C, planes = k.chw ? C : 1;     // elements per pixel in a run, runs per box row
  const int len = cols * inter;

  // ---- stage: every run of this workgroup, read along the run
  for (int seg = 0; seg < rows * planes; ++seg) {
    const int p = seg / planes, pl = seg - p * planes;
    const size_t e0 = k.chw ? ((size_t)pl * k.h + (y0 + p)) * k.w + x0 : ((size_t)(y0 + p) * k.w + x0) * C;
    float(*const out)[kPitch] = stage[p];
    if constexpr (sizeof(SRC) == 4) {
      const float* const run = static_cast<const float*>(k.src) + e0;
      for (int j = tid; j < len; j += kThreads) {
        const int x = div_small(j, inter);
        out[pl + j - x * inter][x] = run[j];
      }
    } else {
      const unsigned char* const run = static_cast<const unsigned char*>(k.src) + e0;
      const int head = min((int)((4 - ((uintptr_t)run & 3)) & 3), len);          // bytes in front of the first aligned dword
      const int nd = (len - head) >> 2, tail = (len - head) & 3;
      for (int d = tid; d < nd; d += kThreads) {
        const unsigned word = *reinterpret_cast<const unsigned*>(run + head + 4 * d);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int j = head + 4 * d + b, x = div_small(j, inter);
          out[pl + j - x * inter][x] = unit_of((word >> (8 * b)) & 255u);
        }
      }
      if (tid < head) {
        const int j = tid, x = div_small(j, inter);
        out[pl + j - x * inter][x] = unit_of(run[j]);
      }
      if (tid < tail) {
        const int j = head + 4 * nd + tid, x = div_small(j, inter);
        out[pl + j - x * inter][x] = unit_of(run[j]);
      }
    }
  }
  __syncthreads();

  // ---- store: (row, channel) -> one destination row of `cols` floats; unit 0 = the scalars in front of the row's 16-byte grid,
  //      units 1..nq = its quads, the last unit = the scalars behind it
  const int U = (cols >> 2) + 2;
  for (int i = tid; i < rows * C * U; i += kThreads) {
    const int rr = i / U, u = i - rr * U;
    const int p = rr / C, ch = rr - p * C;
    float* const row = k.dst + (((size_t)tile * C + ch) * k.th + (r0 + p)) * k.tw + c0;
    const float* const s = stage[p][ch];
    const int head = min((int)((4 - (((uintptr_t)row >> 2) & 3)) & 3), cols);
    const int nq = (cols - head) >> 2, tail = (cols - head) & 3;
    if (u == 0) {
      for (int x = 0; x < head; ++x) row[x] = s[x];
    } else if (u <= nq) {
      const int x = head + 4 * (u - 1);
      float4 v;
      v.x = s[x]; v.y = s[x + 1]; v.z = s[x + 2]; v.w = s[x + 3];
      *reinterpret_cast<float4*>(row + x) = v;
    } else if (u == U - 1) {
      for (int x = cols - tail; x < cols; ++x) row[x] = s[x];
    }
  }
}

struct BlendArgs {
  const float* tiles;                    // [ny * nx][c][th][tw]
  const int* ri;                         // row slots [kSlots][rp]: tile row, -1 = unused
  const float* rw;
  const int* ci;                         // column slots [kSlots][cp]
  const float* cw;
  void* dst;                             // [ho][wo][c] or [c][ho][wo]
  int rp, cp, ny, nx, th, tw, step_y, last_y, step_x, last_x, ho, wo, chw, clip, vec, xblocks;
};

template <typename DST>
__device__ __forceinline__ DST finish(float v, int clip);
template <>
__device__ __forceinline__ unsigned char finish<unsigned char>(float v, int) { return (unsigned char)virnet::quant_u8(v); }
template <>
__device__ __forceinline__ float finish<float>(float v, int clip) {                    // np.clip: -0 and NaN pass
  return clip ? (v < 0.f ? 0.f : (v > 1.f ? 1.f : v)) : v;
}

template <typename DST, int C, bool CROP>
__global__ __launch_bounds__(kThreads) void tile_blend_kernel(const BlendArgs k) {
  const int qy = blockIdx.x / k.xblocks, xb = blockIdx.x - qy * k.xblocks;
  const int qx = (xb * kThreads + threadIdx.x) * kPx;
  if (qx >= k.wo) return;
  constexpr int S = CROP ? 1 : kSlots;
  const int per_tile = C * k.th * k.tw;                                       // < 2^31 (host check)

  // row slots: the same for the whole workgroup
  int ty[S], ly[S];
  float wy[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int t = k.ri[s * k.rp + qy];
    const int l = qy - min(t * k.step_y, k.last_y);
    ty[s] = ((unsigned)t < (unsigned)k.ny && (unsigned)l < (unsigned)k.th) ? t : -1;
    ly[s] = l;
    wy[s] = k.rw[s * k.rp + qy];
  }
  // column slots of the four pixels (pitch and qx are multiples of four: one 16-byte load per slot)
  int tx[S][kPx], lx[S][kPx];
  float wx[S][kPx];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int4 t4 = *reinterpret_cast<const int4*>(k.ci + s * k.cp + qx);
    const float4 w4 = *reinterpret_cast<const float4*>(k.cw + s * k.cp + qx);
    const int t[kPx] = {t4.x, t4.y, t4.z, t4.w};
    const float w[kPx] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
    for (int i = 0; i < kPx; ++i) {
      const int l = qx + i - min(t[i] * k.step_x, k.last_x);
      tx[s][i] = ((unsigned)t[i] < (unsigned)k.nx && (unsigned)l < (unsigned)k.tw && qx + i < k.wo) ? t[i] : -1;
      lx[s][i] = l;
      wx[s][i] = w[i];
    }
  }

  float acc[kPx][C];
#pragma unroll
  for (int i = 0; i < kPx; ++i)
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[i][ch] = 0.f;
#pragma unroll
  for (int sy = 0; sy < S; ++sy) {
    if (ty[sy] < 0) continue;
#pragma unroll
    for (int sx = 0; sx < S; ++sx) {
#pragma unroll
      for (int i = 0; i < kPx; ++i) {
        if (tx[sx][i] < 0) continue;
        const float* const base = k.tiles + (size_t)(ty[sy] * k.nx + tx[sx][i]) * per_tile;
        const int at = ly[sy] * k.tw + lx[sx][i];
        const float wgt = wy[sy] * wx[sx][i];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
          const float v = base[ch * k.th * k.tw + at];
          if (CROP) acc[i][ch] = v;
          else acc[i][ch] = acc[i][ch] + wgt * v;
        }
      }
    }
  }

  DST o[kPx][C];
#pragma unroll
  for (int i = 0; i < kPx; ++i)
#pragma unroll
    for (int ch = 0; ch < C; ++ch) o[i][ch] = finish<DST>(acc[i][ch], k.clip);

  DST* const dst = static_cast<DST*>(k.dst);
  const int plane = k.ho * k.wo, px0 = qy * k.wo + qx;                        // ho * wo * c < 2^31 (host check)
  if (k.vec) {                                                                // wo % 4 == 0: all four pixels exist, every run is aligned
    if (k.chw) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        if constexpr (sizeof(DST) == 4) {
          float4 v;
          v.x = o[0][ch]; v.y = o[1][ch]; v.z = o[2][ch]; v.w = o[3][ch];
          *reinterpret_cast<float4*>(dst + ch * plane + px0) = v;
        } else {
          *reinterpret_cast<unsigned*>(dst + ch * plane + px0) =
              (unsigned)o[0][ch] | ((unsigned)o[1][ch] << 8) | ((unsigned)o[2][ch] << 16) | ((unsigned)o[3][ch] << 24);
        }
      }
    } else {
      DST flat[kPx * C];
#pragma unroll
      for (int i = 0; i < kPx; ++i)
#pragma unroll
        for (int ch = 0; ch < C; ++ch) flat[i * C + ch] = o[i][ch];
#pragma unroll
      for (int q = 0; q < C; ++q) {
        if constexpr (sizeof(DST) == 4) {
          float4 v;
          v.x = flat[4 * q]; v.y = flat[4 * q + 1]; v.z = flat[4 * q + 2]; v.w = flat[4 * q + 3];
          *reinterpret_cast<float4*>(dst + px0 * C + 4 * q) = v;
        } else {
          *reinterpret_cast<unsigned*>(dst + px0 * C + 4 * q) = (unsigned)flat[4 * q] | ((unsigned)flat[4 * q + 1] << 8) |
                                                               ((unsigned)flat[4 * q + 2] << 16) | ((unsigned)flat[4 * q + 3] << 24);
        }
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < kPx; ++i) {
    if (qx + i >= k.wo) continue;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      if (k.chw) dst[ch * plane + px0 + i] = o[i][ch];
      else dst[(px0 + i) * C + ch] = o[i][ch];
    }
  }
}

template <typename DST, int C>
void launch_blend_c(bool crop, dim3 grid, hipStream_t s, const BlendArgs& k) {
  if (crop) hipLaunchKernelGGL((tile_blend_kernel<DST, C, true>), grid, dim3(kThreads), 0, s, k);
  else hipLaunchKernelGGL((tile_blend_kernel<DST, C, false>), grid, dim3(kThreads), 0, s, k);
}

template <typename DST>
void launch_blend(int c, bool crop, dim3 grid, hipStream_t s, const BlendArgs& k) {
  switch (c) {
    case 1: launch_blend_c<DST, 1>(crop, grid, s, k); break;
    case 2: launch_blend_c<DST, 2>(crop, grid, s, k); break;
    case 3: launch_blend_c<DST, 3>(crop, grid, s, k); break;
    default: launch_blend_c<DST, 4>(crop, grid, s, k); break;
  }
}

}  // namespace

extern "C" int virnet_tile_gather(const void* src, int src_is_f32, int src_chw, int h, int w, int c, const int* boxes, int n, int th, int tw,
                                  float* dst, void* stream) {
  VIRNET_REQUIRE(src && dst && boxes, "virnet_tile_gather: NULL pointer");
  VIRNET_REQUIRE(c >= 1 && c <= kMaxC, "virnet_tile_gather: %d channels (1..%d expected)", c, kMaxC);
  VIRNET_REQUIRE(h > 0 && w > 0 && (long long)h * w * c < (1ll << 31), "virnet_tile_gather: image %dx%dx%d is empty or reaches 2^31 elements", h, w, c);
  VIRNET_REQUIRE(n >= 1 && n <= VIRNET_TILE_BOXES, "virnet_tile_gather: %d boxes in one launch (1..%d expected)", n, VIRNET_TILE_BOXES);
  VIRNET_REQUIRE(th >= 1 && th <= h && tw >= 1 && tw <= w, "virnet_tile_gather: box %dx%d does not fit the image %dx%d", th, tw, h, w);
  VIRNET_REQUIRE((long long)n * c * th * tw < (1ll << 31), "virnet_tile_gather: %d boxes of %dx%dx%d reach 2^31 elements", n, c, th, tw);
  VIRNET_REQUIRE(((uintptr_t)dst & 3) == 0 && (!src_is_f32 || ((uintptr_t)src & 3) == 0), "virnet_tile_gather: misaligned float32 tensor");
  GatherArgs k{};
  k.src = src; k.dst = dst; k.h = h; k.w = w; k.c = c; k.chw = src_chw != 0; k.th = th; k.tw = tw;
  k.xchunks = (tw + kChunk - 1) / kChunk;
  for (int i = 0; i < n; ++i) {
    const int y = boxes[2 * i], x = boxes[2 * i + 1];
    VIRNET_REQUIRE(y >= 0 && y <= h - th && x >= 0 && x <= w - tw, "virnet_tile_gather: box %d at (%d, %d) of size %dx%d leaves the image %dx%d", i, y,
                   x, th, tw, h, w);
    k.box[i][0] = y; k.box[i][1] = x;
  }
  const long long gx = (long long)k.xchunks * ((th + kRows - 1) / kRows);
  VIRNET_REQUIRE(gx <= 0x7fffffffll, "virnet_tile_gather: box %dx%d is too large (%lld workgroups)", th, tw, gx);
  const dim3 grid((unsigned)gx, n);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (src_is_f32) hipLaunchKernelGGL(tile_gather_kernel<float>, grid, dim3(kThreads), 0, s, k);
  else hipLaunchKernelGGL(tile_gather_kernel<unsigned char>, grid, dim3(kThreads), 0, s, k);
  return virnet::check_launch("tile_gather launch");
}

extern "C" int virnet_tile_blend(const float* tiles, const int* row_idx, const float* row_w, const int* col_idx, const float* col_w, int row_pitch,
                                 int col_pitch, int ny, int nx, int c, int th, int tw, int step_y, int last_y, int step_x, int last_x, int ho,
                                 int wo, void* dst, int dst_is_f32, int chw, int clip, int crop, void* stream) {
  VIRNET_REQUIRE(tiles && row_idx && row_w && col_idx && col_w && dst, "virnet_tile_blend: NULL pointer");
  VIRNET_REQUIRE(c >= 1 && c <= kMaxC, "virnet_tile_blend: %d channels (1..%d expected)", c, kMaxC);
  VIRNET_REQUIRE(ny >= 1 && nx >= 1 && th >= 1 && tw >= 1, "virnet_tile_blend: empty stack (%d x %d tiles of %dx%d)", ny, nx, th, tw);
  VIRNET_REQUIRE((long long)ny * nx * c * th * tw < (1ll << 31), "virnet_tile_blend: the stack of %d x %d tiles of %dx%dx%d reaches 2^31 elements", ny,
                 nx, c, th, tw);
  VIRNET_REQUIRE(ho >= th && wo >= tw && (long long)ho * wo * c < (1ll << 31), "virnet_tile_blend: output %dx%dx%d is smaller than a tile %dx%d or reaches 2^31 elements",
                 ho, wo, c, th, tw);
  VIRNET_REQUIRE(step_y >= 0 && step_x >= 0 && last_y == ho - th && last_x == wo - tw,
                 "virnet_tile_blend: steps (%d, %d) / last starts (%d, %d) do not describe a %dx%d grid of %dx%d tiles", step_y, step_x, last_y, last_x, ho,
                 wo, th, tw);
  VIRNET_REQUIRE((long long)(ny - 1) * step_y < (1ll << 31) && (long long)(nx - 1) * step_x < (1ll << 31), "virnet_tile_blend: steps (%d, %d) are too large",
                 step_y, step_x);
  VIRNET_REQUIRE(row_pitch >= ho && col_pitch >= wo && row_pitch % 4 == 0 && col_pitch % 4 == 0,
                 "virnet_tile_blend: table pitches (%d, %d) must be multiples of four and cover the output %dx%d", row_pitch, col_pitch, ho, wo);
  VIRNET_REQUIRE((((uintptr_t)row_idx | (uintptr_t)row_w | (uintptr_t)col_idx | (uintptr_t)col_w) & 15) == 0, "virnet_tile_blend: tap tables must be 16-byte aligned");
  VIRNET_REQUIRE(((uintptr_t)tiles & 3) == 0 && (!dst_is_f32 || ((uintptr_t)dst & 3) == 0), "virnet_tile_blend: misaligned float32 tensor");
  BlendArgs k{};
  k.tiles = tiles; k.ri = row_idx; k.rw = row_w; k.ci = col_idx; k.cw = col_w; k.dst = dst;
  k.rp = row_pitch; k.cp = col_pitch; k.ny = ny; k.nx = nx; k.th = th; k.tw = tw;
  k.step_y = step_y; k.last_y = last_y; k.step_x = step_x; k.last_x = last_x; k.ho = ho; k.wo = wo;
  k.chw = chw != 0; k.clip = clip != 0;
  k.vec = wo % 4 == 0 && ((uintptr_t)dst & (dst_is_f32 ? 15 : 3)) == 0;
  k.xblocks = (wo + kThreads * kPx - 1) / (kThreads * kPx);
  const long long gx = (long long)k.xblocks * ho;
  VIRNET_REQUIRE(gx <= 0x7fffffffll, "virnet_tile_blend: output %dx%d is too large (%lld workgroups)", ho, wo, gx);
  const dim3 grid((unsigned)gx);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dst_is_f32) launch_blend<float>(c, crop != 0, grid, s, k);
  else launch_blend<unsigned char>(c, crop != 0, grid, s, k);
  return virnet::check_launch("tile_blend launch");
}
