// The JPEG round trip of the SISR degradation on the device (virnet_amd/jpeg.py states the algorithm, step by step; jpeg.roundtrip_np is the
// definition): baseline 4:2:0 with libjpeg's defaults, without the entropy coding, in 32-bit integers.  Two launches around a uint8
// workspace that holds, per sample, the decoded Y' plane [h][w] and the decoded Cb', Cr' planes [hc][wc] (hc = ceil(h/2), wc = ceil(w/2)):
//
//   jpeg_blocks_kernel   one wave per 16 x 16 MCU: loads the pixels (edge-clamped: the replication padding), converts them to YCbCr into
//                        LDS, and runs forward DCT -> quantise -> dequantise -> inverse DCT on the MCU's six 8 x 8 blocks, four of Y and
//                        one each of the 2 x 2-downsampled Cb and Cr.  48 lanes hold one block row each in registers; the two transposes
//                        of a block go through LDS (pitch 9 words).  The decoded samples that lie inside the image go to the workspace.
//   jpeg_finish_kernel   four output pixels of a row per thread: "fancy" chroma upsample from the workspace (the one-sample halo that
//                        crosses MCU borders is why this is a launch of its own), YCbCr -> RGB, store as uint8 or fp32.
//
// A sample whose quality is 0 (or negative) is not compressed: the first kernel leaves it alone and the second copies the input through.
// No atomics, no scratch; a sample's result depends on that sample alone.
#include "common.h"
#include "../../include/virnet_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMcuThreads = 64;
constexpr int kFinishThreads = 256;
constexpr int kPitch = 9;                    // words per block row in LDS: the column reads of a transpose hit eight different banks

constexpr int fix16(double x) { return (int)(x * 65536.0 + 0.5); }

// 13 constant bits, 2 pass-1 bits
constexpr int kConstBits = 13, kPass1Bits = 2;
constexpr int F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633;
constexpr int F1_501 = 12299, F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;

struct JpegArgs {
  const void* src;
  void* dst;
  const int* qf;
  const int* tables;         // [101][2][64]
  unsigned char* ws;
  int src_f32, dst_f32;
  int h, w, hc, wc;
};

// eval.img_as_ubyte, as csrc/metrics.hip's quant_u8 states it: clamp in fp32, times 255 in fp64 (exact), round half to even
__device__ __forceinline__ int quant_u8(float x) {
  const float c = x > 0.f ? (x < 1.f ? x : 1.f) : 0.f;       // NaN and -0 -> +0
  return (int)rint((double)c * 255.0);
}

__device__ __forceinline__ int load_u8(const void* base, size_t o, int f32) {
  return f32 ? quant_u8(static_cast<const float*>(base)[o]) : (int)static_cast<const unsigned char*>(base)[o];
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
__device__ __forceinline__ int clip255(int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }

template <bool FIRST>
__device__ __forceinline__ void fdct_pass(int (&d)[8]) {
  constexpr int n = FIRST ? kConstBits - kPass1Bits : kConstBits + kPass1Bits;
  int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (FIRST) {
    d[0] = (t10 + t11) * (1 << kPass1Bits);
    d[4] = (t10 - t11) * (1 << kPass1Bits);
  } else {
    d[0] = descale(t10 + t11, kPass1Bits);
    d[4] = descale(t10 - t11, kPass1Bits);
  }
  int z1 = (t12 + t13) * F0_541;
  d[2] = descale(z1 + t13 * F0_765, n);
  d[6] = descale(z1 - t12 * F1_847, n);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * F1_175;
  t4 *= F0_298; t5 *= F2_053; t6 *= F3_072; t7 *= F1_501;
  z1 *= -F0_899; z2 *= -F2_562;
  z3 = z3 * -F1_961 + z5;
  z4 = z4 * -F0_390 + z5;
  d[7] = descale(t4 + z1 + z3, n);
  d[5] = descale(t5 + z2 + z4, n);
  d[3] = descale(t6 + z2 + z3, n);
  d[1] = descale(t7 + z1 + z4, n);
}

__device__ __forceinline__ void idct_pass(int (&c)[8], int n) {
  int z1 = (c[2] + c[6]) * F0_541;
  int t2 = z1 - c[6] * F1_847, t3 = z1 + c[2] * F0_765;
  int t0 = (c[0] + c[4]) * (1 << kConstBits), t1 = (c[0] - c[4]) * (1 << kConstBits);
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = c[7]; t1 = c[5]; t2 = c[3]; t3 = c[1];
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * F1_175;
  t0 *= F0_298; t1 *= F2_053; t2 *= F3_072; t3 *= F1_501;
  z1 *= -F0_899; z2 *= -F2_562;
  z3 = z3 * -F1_961 + z5;
  z4 = z4 * -F0_390 + z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  c[0] = descale(t10 + t3, n); c[7] = descale(t10 - t3, n);
  c[1] = descale(t11 + t2, n); c[6] = descale(t11 - t2, n);
  c[2] = descale(t12 + t1, n); c[5] = descale(t12 - t1, n);
  c[3] = descale(t13 + t0, n); c[4] = descale(t13 - t0, n);
}

__global__ __launch_bounds__(kMcuThreads) void jpeg_blocks_kernel(const JpegArgs a) {
  const int b = blockIdx.z;
  int q = a.qf[b];
  if (q <= 0) return;                                        // (uniform over the workgroup)
  q = q > 100 ? 100 : q;
  __shared__ int ycc[3][16][17];                             // the MCU's pixels as Y, Cb, Cr at full resolution
  __shared__ int tr[6][8][kPitch];
  const int lane = threadIdx.x;
  const int y0 = blockIdx.y * 16, x0 = blockIdx.x * 16;
  const size_t plane = (size_t)a.h * a.w;
  {
    const int r = lane >> 2, c0 = (lane & 3) * 4;
    const int sy = min(y0 + r, a.h - 1);
    const size_t row = (size_t)b * 3 * plane + (size_t)sy * a.w;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const size_t o = row + min(x0 + c0 + e, a.w - 1);
      const int R = load_u8(a.src, o, a.src_f32), G = load_u8(a.src, o + plane, a.src_f32), B = load_u8(a.src, o + 2 * plane, a.src_f32);
      ycc[0][r][c0 + e] = (fix16(.299) * R + fix16(.587) * G + fix16(.114) * B + 32768) >> 16;
      ycc[1][r][c0 + e] = (-fix16(.16874) * R - fix16(.33126) * G + 32768 * B + (128 << 16) + 32767) >> 16;
      ycc[2][r][c0 + e] = (32768 * R - fix16(.41869) * G - fix16(.08131) * B + (128 << 16) + 32767) >> 16;
    }
  }
  __syncthreads();
  const int blk = lane >> 3, r = lane & 7;                   // lanes 0..47: one row (then one column, then one row) of block blk
  const bool work = blk < 6;
  const int comp = blk < 4 ? 0 : blk - 3;
  int d[8];
  if (work) {
    if (comp == 0) {
      const int yr = (blk >> 1) * 8 + r, xc = (blk & 1) * 8;
#pragma unroll
      for (int k = 0; k < 8; ++k) d[k] = ycc[0][yr][xc + k] - 128;
    } else {
      // rows past the last downsampled row repeat it (not the downsampling of repeated full-resolution rows)
      const int rr = 2 * (min((y0 >> 1) + r, a.hc - 1) - (y0 >> 1));
#pragma unroll
      for (int k = 0; k < 8; ++k)
        d[k] = ((ycc[comp][rr][2 * k] + ycc[comp][rr][2 * k + 1] + ycc[comp][rr + 1][2 * k] + ycc[comp][rr + 1][2 * k + 1] + 1 + (k & 1)) >> 2) - 128;
    }
    fdct_pass<true>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) tr[blk][r][k] = d[k];
  }
  __syncthreads();
  if (work) {
    const int* tab = a.tables + ((size_t)q * 2 + (comp ? 1 : 0)) * 64;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = tr[blk][k][r];
    fdct_pass<false>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int qv = tab[k * 8 + r];
      const unsigned div = (unsigned)qv * 8u;
      const unsigned mag = ((unsigned)abs(d[k]) + (div >> 1)) / div;      // exact integer division
      d[k] = (d[k] < 0 ? -(int)mag : (int)mag) * qv;
    }
    idct_pass(d, kConstBits - kPass1Bits);
#pragma unroll
    for (int k = 0; k < 8; ++k) tr[blk][k][r] = d[k];        // (column r of the block is read and written by this lane only)
  }
  __syncthreads();
  if (work) {
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = tr[blk][r][k];
    idct_pass(d, kConstBits + kPass1Bits + 3);
    const size_t cplane = (size_t)a.hc * a.wc;
    unsigned char* out = a.ws + (size_t)b * (plane + 2 * cplane);
    int gy, gx, ph, pw;
    if (comp == 0) {
      gy = y0 + (blk >> 1) * 8 + r; gx = x0 + (blk & 1) * 8; ph = a.h; pw = a.w;
    } else {
      out += plane + (size_t)(comp - 1) * cplane;
      gy = (y0 >> 1) + r; gx = x0 >> 1; ph = a.hc; pw = a.wc;
    }
    if (gy < ph) {
      out += (size_t)gy * pw + gx;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (gx + k < pw) out[k] = (unsigned char)clip255(d[k] + 128);
    }
  }
}

__device__ __forceinline__ void store4(const JpegArgs& a, size_t o, const int (&v)[4], int cnt) {
  if (a.dst_f32) {
    float* p = static_cast<float*>(a.dst) + o;
    const float s = (float)(1.0 / 255.0);                    // eval.img_as_float32: one fp32 multiply
    if (cnt == 4 && ((uintptr_t)p & 15) == 0) {
      *reinterpret_cast<float4*>(p) = make_float4((float)v[0] * s, (float)v[1] * s, (float)v[2] * s, (float)v[3] * s);
    } else {
      for (int e = 0; e < cnt; ++e) p[e] = (float)v[e] * s;
    }
  } else {
    unsigned char* p = static_cast<unsigned char*>(a.dst) + o;
    if (cnt == 4 && ((uintptr_t)p & 3) == 0) {
      *reinterpret_cast<unsigned*>(p) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
    } else {
      for (int e = 0; e < cnt; ++e) p[e] = (unsigned char)v[e];
    }
  }
}

__global__ __launch_bounds__(kFinishThreads) void jpeg_finish_kernel(const JpegArgs a) {
  const int b = blockIdx.y;
  const int quads = (a.w + 3) >> 2;
  const int idx = blockIdx.x * kFinishThreads + threadIdx.x;
  if (idx >= a.h * quads) return;
  const int y = idx / quads, x = (idx - y * quads) * 4;
  const int cnt = min(4, a.w - x);
  const size_t plane = (size_t)a.h * a.w;
  const size_t o = (size_t)b * 3 * plane + (size_t)y * a.w + x;
  if (a.qf[b] <= 0) {                                        // not compressed: the input as it is
    for (int ch = 0; ch < 3; ++ch) {
      const size_t oc = o + ch * plane;
      if (a.src_f32 && a.dst_f32) {
        for (int e = 0; e < cnt; ++e) static_cast<float*>(a.dst)[oc + e] = static_cast<const float*>(a.src)[oc + e];
      } else {
        int v[4] = {0, 0, 0, 0};
        for (int e = 0; e < cnt; ++e) v[e] = load_u8(a.src, oc + e, a.src_f32);
        store4(a, oc, v, cnt);
      }
    }
    return;
  }
  const size_t cplane = (size_t)a.hc * a.wc;
  const unsigned char* yp = a.ws + (size_t)b * (plane + 2 * cplane);
  const unsigned char* cp = yp + plane;
  const int i = y >> 1;
  const int far = (y & 1) ? min(i + 1, a.hc - 1) : max(i - 1, 0);
  const int j0 = x >> 1;
  int cc[2][4];                                              // Cb', Cr' of the four pixels
  for (int comp = 0; comp < 2; ++comp) {
    const unsigned char* near_row = cp + comp * cplane + (size_t)i * a.wc;
    const unsigned char* far_row = cp + comp * cplane + (size_t)far * a.wc;
    if (a.wc <= 2) {                                         // the library repeats the samples of planes this narrow
#pragma unroll
      for (int e = 0; e < 4; ++e) cc[comp][e] = near_row[min(j0 + (e >> 1), a.wc - 1)];
    } else {
      int v[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int j = min(max(j0 - 1 + t, 0), a.wc - 1);
        v[t] = 3 * near_row[j] + far_row[j];
      }
      cc[comp][0] = (3 * v[1] + v[0] + 8) >> 4;              // (the clamp makes the first and last columns their own neighbours)
      cc[comp][1] = (3 * v[1] + v[2] + 7) >> 4;
      cc[comp][2] = (3 * v[2] + v[1] + 8) >> 4;
      cc[comp][3] = (3 * v[2] + v[3] + 7) >> 4;
    }
  }
  int R[4] = {0, 0, 0, 0}, G[4] = {0, 0, 0, 0}, B[4] = {0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e < cnt) {
      const int Y = yp[(size_t)y * a.w + x + e], cb = cc[0][e] - 128, cr = cc[1][e] - 128;
      R[e] = clip255(Y + ((fix16(1.402) * cr + 32768) >> 16));
      G[e] = clip255(Y + ((-fix16(.34414) * cb - fix16(.71414) * cr + 32768) >> 16));
      B[e] = clip255(Y + ((fix16(1.772) * cb + 32768) >> 16));
    }
  }
  store4(a, o, R, cnt);
  store4(a, o + plane, G, cnt);
  store4(a, o + 2 * plane, B, cnt);
}

bool sizes_ok(int n, int h, int w) { return n >= 1 && n <= 65535 && h >= 1 && w >= 1 && h <= 32768 && w <= 32768; }

}  // namespace

extern "C" size_t virnet_jpeg_workspace_bytes(int n, int h, int w) {
  if (!sizes_ok(n, h, w)) return 0;
  const size_t hc = (size_t)(h + 1) / 2, wc = (size_t)(w + 1) / 2;
  return (size_t)n * ((size_t)h * w + 2 * hc * wc);
}

extern "C" int virnet_jpeg_roundtrip(const void* src, int src_is_f32, void* dst, int dst_is_f32, const int32_t* qf, const int32_t* tables,
                                     void* workspace, int n, int h, int w, void* stream) {
  VIRNET_REQUIRE(src && dst && qf && tables && workspace, "virnet_jpeg_roundtrip: NULL pointer");
  VIRNET_REQUIRE(sizes_ok(n, h, w), "virnet_jpeg_roundtrip: n %d outside 1..65535 or image %dx%d outside 1..32768", n, h, w);
  JpegArgs a;
  a.src = src; a.dst = dst; a.qf = qf; a.tables = tables; a.ws = static_cast<unsigned char*>(workspace);
  a.src_f32 = src_is_f32 != 0; a.dst_f32 = dst_is_f32 != 0;
  a.h = h; a.w = w; a.hc = (h + 1) / 2; a.wc = (w + 1) / 2;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(jpeg_blocks_kernel, dim3((w + 15) / 16, (h + 15) / 16, n), dim3(kMcuThreads), 0, s, a);
  if (int rc = virnet::check_launch("jpeg blocks launch")) return rc;
  const long long quads = (long long)h * ((w + 3) / 4);
  hipLaunchKernelGGL(jpeg_finish_kernel, dim3((unsigned)((quads + kFinishThreads - 1) / kFinishThreads), n), dim3(kFinishThreads), 0, s, a);
  return virnet::check_launch("jpeg finish launch");
}
