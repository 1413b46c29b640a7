// elbo.hip -- the denoising objective and its variance prior on the device (host definitions: virnet_amd/loss.py elbo_denoising_simple,
// reference loss/ELBO_simple.py:12-53; utils/util_denoising.py:24-63 noise_estimate_fun).  Dense NCHW fp32 tensors.
//
//   elbo_value_kernel<V, CT>  one pass over the pixels: a thread owns V (4: 16-byte accesses, 1: any size and alignment) pixels adjacent
//                             in x of one sample and loops over the channels, so the broadcasts of a one-channel sigma_est / beta0 stay
//                             in registers.  Per element, in fp32 with the accurate logf and IEEE division:
//                               lh        0.5 * (log(beta) - psi + (a / beta) * ((x - mu)^2 + eps2)),  beta = sigma_est * alpha0, a = alpha0 - 1
//                               kl_gauss  (mu - gt)^2 / eps2
//                               kl_Igamma a * (beta0 / beta - 1) + a * (log(beta) - log(beta0))         over max(Cs, Cb) channels
//                             each added to a per-thread fp64 sum; wave reduction (shuffles), the block's four waves through LDS, one
//                             (lh, kl_gauss, kl_Igamma) fp64 partial per block to the workspace.
//   elbo_finish_kernel        one block adds the partials in index order (thread t: t, t + 256, ...; then the same tree), divides by the
//                             element counts and writes loss, lh, kl_gauss, kl_Igamma as four floats.
//   elbo_grad_kernel<V, CT>   same traversal, closed form, times the upstream scalar read from device memory:
//                               dmu    = g wd / M * ((a / beta) (mu - x) + (mu - gt) / eps2)
//                               dsigma = alpha0 * (g wd / M * 0.5 * sum_c (1 / beta - a S_c / beta^2) + g wk / Mk * a * sum_j (1 / beta - beta0_j / beta^2))
//                             S_c = (x - mu)^2 + eps2; the sums run over the channels broadcast against this sigma channel; M = N C H W,
//                             Mk = N max(Cs, Cb) H W; wd, wk: host weights of the data terms and of the variance term (deep supervision).
//   noise_estimate_kernel     out = max(G_k (*) (noisy - gt)^2, floor), reflect border: one workgroup per 16 x 64 tile of one plane stages
//                             the squared error of the tile and its halo in LDS (fp64, squared on load), filters rows, then columns.
//
// No atomics anywhere: every sum has one fixed order that depends on the shape only, so results are bitwise reproducible.
#include "common.h"
#include "../../include/virnet_hip.h"

#include <cstdint>
#include <initializer_list>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;          // value / gradient grid: four workgroups on each of the 256 CUs; 24 KB of partials at most
constexpr int kNeTy = 16, kNeTx = 64;     // noise-estimate tile of output pixels
constexpr int kNeMaxK = 31;

struct ElboArgs {
  const float *mu, *sigma, *noisy, *gt, *beta0;
  const float *alpha0, *psi;      // device scalars
  const float* gout;              // gradient: upstream scalar (device)
  float *dmu, *dsigma;            // gradient
  double* part;                   // value: [blocks][3]
  int c, cs, cb;
  unsigned hw, gpp, items;        // pixels per plane, thread items per plane (hw / V), items in all (n * gpp)
  float eps2;
  int with_klig;
  double wd, wk;                  // gradient: weights over the element counts, wd / M and wk / Mk
};

template <int V>
__device__ __forceinline__ void load(const float* p, float (&r)[V]) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
  } else {
    r[0] = *p;
  }
}

template <int V>
__device__ __forceinline__ void store(float* p, const float (&r)[V]) {
  if constexpr (V == 4)
    *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
  else
    *p = r[0];
}

// sum over the block in a fixed order: lanes by shuffle tree, then waves 0..3; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int tid = threadIdx.x;
  __syncthreads();                       // (red may still be read from the previous sum)
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

template <int V, int CT>
__global__ __launch_bounds__(kThreads) void elbo_value_kernel(const ElboArgs a) {
  __shared__ double red[kThreads / 64];
  const int C = CT ? CT : a.c;
  constexpr int kUnroll = CT ? CT : 1;      // a run-time channel count stays a loop
  const bool sig_pc = a.cs > 1, b0_pc = a.cb > 1, klig = a.with_klig != 0;
  const float alpha = *a.alpha0, psi = *a.psi, am1 = alpha - 1.f, eps2 = a.eps2;
  const size_t hw = a.hw;
  double s_lh = 0.0, s_kg = 0.0, s_ki = 0.0;
  for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < a.items; i += gridDim.x * kThreads) {
    const unsigned n = i / a.gpp;
    const size_t p = (size_t)(i - n * a.gpp) * V;
    const size_t img = (size_t)n * C * hw + p;
    const float* const sg = a.sigma + (size_t)n * a.cs * hw + p;
    const float* const b0 = a.beta0 + (size_t)n * a.cb * hw + p;
    float lb[V], q[V], beta[V], bz[V], lbz[V];
#pragma unroll kUnroll
    for (int c = 0; c < C; ++c) {
      if (c == 0 || sig_pc) {
        float s[V];
        load<V>(sg + c * hw, s);
#pragma unroll
        for (int v = 0; v < V; ++v) {
          beta[v] = s[v] * alpha;
          lb[v] = logf(beta[v]);
          q[v] = am1 / beta[v];
        }
      }
      if (klig && (c == 0 || b0_pc)) {
        load<V>(b0 + c * hw, bz);
#pragma unroll
        for (int v = 0; v < V; ++v) lbz[v] = logf(bz[v]);
      }
      if (klig && (c == 0 || sig_pc || b0_pc)) {
#pragma unroll
        for (int v = 0; v < V; ++v) s_ki += (double)(am1 * (bz[v] / beta[v] - 1.f) + am1 * (lb[v] - lbz[v]));
      }
      float x[V], m[V], g[V];
      load<V>(a.noisy + img + c * hw, x);
      load<V>(a.mu + img + c * hw, m);
      load<V>(a.gt + img + c * hw, g);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const float d = x[v] - m[v], e = m[v] - g[v];
        s_lh += (double)(0.5f * (lb[v] - psi + q[v] * (d * d + eps2)));
        s_kg += (double)(e * e / eps2);
      }
    }
  }
  s_lh = block_sum(s_lh, red);
  s_kg = block_sum(s_kg, red);
  s_ki = block_sum(s_ki, red);
  if (threadIdx.x == 0) {
    double* const dst = a.part + (size_t)blockIdx.x * 3;
    dst[0] = s_lh; dst[1] = s_kg; dst[2] = s_ki;
  }
}

__global__ __launch_bounds__(kThreads) void elbo_finish_kernel(const double* __restrict__ part, int blocks, float* __restrict__ out, double inv_m,
                                                               double inv_mk) {
  __shared__ double red[kThreads / 64];
  double s[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < blocks; b += kThreads) {
    s[0] += part[(size_t)b * 3];
    s[1] += part[(size_t)b * 3 + 1];
    s[2] += part[(size_t)b * 3 + 2];
  }
  const double t_lh = block_sum(s[0], red), t_kg = block_sum(s[1], red), t_ki = block_sum(s[2], red);
  if (threadIdx.x == 0) {
    const float lh = (float)(t_lh * inv_m + 0.91893853320467274178);      // + 0.5 log(2 pi)
    const float kg = (float)(0.5 * t_kg * inv_m);
    const float ki = (float)(t_ki * inv_mk);
    out[0] = lh + kg + ki;
    out[1] = lh; out[2] = kg; out[3] = ki;
  }
}

template <int V, int CT>
__global__ __launch_bounds__(kThreads) void elbo_grad_kernel(const ElboArgs a) {
  const int C = CT ? CT : a.c;
  constexpr int kUnroll = CT ? CT : 1;      // a run-time channel count stays a loop
  const bool sig_pc = a.cs > 1, b0_pc = a.cb > 1;
  const float alpha = *a.alpha0, am1 = alpha - 1.f, eps2 = a.eps2;
  const double g = (double)*a.gout;
  const float cd = (float)(g * a.wd), ck = (float)(g * a.wk);      // the upstream gradient enters as one factor: a power of two scales exactly
  const bool klig = a.wk != 0.0;
  const float n_lh = sig_pc ? 1.f : (float)C, n_ki = (sig_pc || !b0_pc) ? 1.f : (float)C;
  const size_t hw = a.hw;
  for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < a.items; i += gridDim.x * kThreads) {
    const unsigned n = i / a.gpp;
    const size_t p = (size_t)(i - n * a.gpp) * V;
    const size_t img = (size_t)n * C * hw + p;
    const size_t so = (size_t)n * a.cs * hw + p;
    const float* const b0 = a.beta0 + (size_t)n * a.cb * hw + p;
    float ib[V], q[V], bz[V], sum_s[V], sum_b[V];
#pragma unroll
    for (int v = 0; v < V; ++v) bz[v] = 0.f;
#pragma unroll kUnroll
    for (int c = 0; c < C; ++c) {
      if (c == 0 || sig_pc) {
        float s[V];
        load<V>(a.sigma + so + c * hw, s);
#pragma unroll
        for (int v = 0; v < V; ++v) {
          ib[v] = 1.f / (s[v] * alpha);
          q[v] = am1 * ib[v];
          sum_s[v] = 0.f;
          sum_b[v] = 0.f;
        }
      }
      if (klig && (c == 0 || b0_pc)) load<V>(b0 + c * hw, bz);
      if (c == 0 || sig_pc || b0_pc) {
#pragma unroll
        for (int v = 0; v < V; ++v) sum_b[v] += bz[v];
      }
      float x[V], m[V], t[V], dm[V];
      load<V>(a.noisy + img + c * hw, x);
      load<V>(a.mu + img + c * hw, m);
      load<V>(a.gt + img + c * hw, t);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const float d = m[v] - x[v];
        dm[v] = cd * (q[v] * d + (m[v] - t[v]) / eps2);
        sum_s[v] += d * d + eps2;
      }
      store<V>(a.dmu + img + c * hw, dm);
      if (sig_pc || c == C - 1) {
        float ds[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const float part_lh = 0.5f * (n_lh * ib[v] - q[v] * ib[v] * sum_s[v]);
          const float part_ki = am1 * (n_ki * ib[v] - ib[v] * ib[v] * sum_b[v]);
          ds[v] = alpha * (cd * part_lh + ck * part_ki);
        }
        store<V>(a.dsigma + so + (sig_pc ? c : 0) * hw, ds);
      }
    }
  }
}

// ---- variance prior ---------------------------------------------------------------------------------------------------------------------
struct NeArgs {
  const float *noisy, *gt;
  const double* taps;
  float* out;
  int h, w, k, p, tiles_x;
  int pitch, rows;      // LDS tile of squared errors: [rows = kNeTy + 2p][pitch = kNeTx + 2p]
  float floor;
};

// image index that bordered coordinate q (-p <= q < n + p, p < n) reads: d c b | a b c d
__device__ __forceinline__ int reflect(int q, int n) { return q < 0 ? -q : (q >= n ? 2 * n - 2 - q : q); }

__global__ __launch_bounds__(kThreads) void noise_estimate_kernel(const NeArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds_ne[];
  double* const tap = lds_ne;                                 // [32]
  double* const e2 = lds_ne + 32;                             // [rows][pitch]
  double* const rowf = e2 + a.rows * a.pitch;                 // [rows][kNeTx]
  const int tid = threadIdx.x;
  const int tile = blockIdx.x;
  const int ty0 = (tile / a.tiles_x) * kNeTy, tx0 = (tile % a.tiles_x) * kNeTx;
  const size_t plane = (size_t)blockIdx.y * a.h * a.w;
  const float* const xn = a.noisy + plane;
  const float* const xg = a.gt + plane;
  if (tid < a.k) tap[tid] = a.taps[tid];
  for (int i = tid; i < a.rows * a.pitch; i += kThreads) {
    const int ly = i / a.pitch, lx = i - ly * a.pitch;
    const int qy = ty0 - a.p + ly, qx = tx0 - a.p + lx;
    double v = 0.0;                                           // beyond the bordered image: feeds outputs that are not stored
    if (qy < a.h + a.p && qx < a.w + a.p) {
      const size_t o = (size_t)reflect(qy, a.h) * a.w + reflect(qx, a.w);
      const double d = (double)xn[o] - (double)xg[o];
      v = d * d;
    }
    e2[i] = v;
  }
  __syncthreads();
  for (int i = tid; i < a.rows * kNeTx; i += kThreads) {
    const int ly = i / kNeTx, x = i - ly * kNeTx;
    const double* const src = e2 + ly * a.pitch + x;
    double s = 0.0;
    for (int v = 0; v < a.k; ++v) s = fma(tap[v], src[v], s);
    rowf[i] = s;
  }
  __syncthreads();
  const int x = tid & (kNeTx - 1), ox = tx0 + x;
#pragma unroll
  for (int j = 0; j < kNeTy * kNeTx / kThreads; ++j) {
    const int y = (tid >> 6) + j * (kThreads / kNeTx), oy = ty0 + y;
    const double* const src = rowf + y * kNeTx + x;
    double s = 0.0;
    for (int u = 0; u < a.k; ++u) s = fma(tap[u], src[u * kNeTx], s);
    if (oy < a.h && ox < a.w) {
      const float r = (float)s;
      a.out[plane + (size_t)oy * a.w + ox] = r > a.floor ? r : a.floor;
    }
  }
}

// 0 when the objective is defined for these sizes (error slot set otherwise)
int elbo_geometry(const char* who, int n, int c, int cs, int cb, int h, int w) {
  VIRNET_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0, "%s: sizes n=%d c=%d h=%d w=%d must be positive", who, n, c, h, w);
  VIRNET_REQUIRE(c <= 65535, "%s: %d channels (1..65535 expected)", who, c);
  VIRNET_REQUIRE(cs == 1 || cs == c, "%s: sigma_est has %d channels (1 or %d expected)", who, cs, c);
  VIRNET_REQUIRE(cb == 1 || cb == c, "%s: beta0 has %d channels (1 or %d expected)", who, cb, c);
  VIRNET_REQUIRE(h <= (1 << 15) && w <= (1 << 15) && (long long)n * h * w < (1ll << 31), "%s: n*h*w = %d*%d*%d must stay below 2^31", who, n, h, w);
  return 0;
}

int elbo_blocks(unsigned items) {
  const unsigned b = (items + kThreads - 1) / kThreads;
  return (int)(b < (unsigned)kMaxBlocks ? b : (unsigned)kMaxBlocks);
}

bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if ((uintptr_t)p & 15) return false;
  return true;
}

bool aligned4(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if ((uintptr_t)p & 3) return false;
  return true;
}

template <typename F4_3, typename F4_0, typename F1_3, typename F1_0>
void dispatch(bool vec, int c, F4_3 f43, F4_0 f40, F1_3 f13, F1_0 f10) {
  if (vec) {
    if (c == 3) f43(); else f40();
  } else {
    if (c == 3) f13(); else f10();
  }
}

}  // namespace

extern "C" size_t virnet_elbo_workspace_bytes(int n, int c, int h, int w) {
  if (elbo_geometry("virnet_elbo_workspace_bytes", n, c, 1, 1, h, w)) return 0;
  return (size_t)elbo_blocks((unsigned)n * (unsigned)(h * w)) * 3 * sizeof(double);      // (the 16-byte form launches a quarter of the items)
}

extern "C" int virnet_elbo_value(const float* mu, const float* sigma_est, const float* im_noisy, const float* im_gt, const float* beta0,
                                 const float* alpha0, const float* psi, float eps2, int with_klig, void* workspace, float* out4, int n, int c,
                                 int cs, int cb, int h, int w, void* stream) {
  VIRNET_REQUIRE(mu && sigma_est && im_noisy && im_gt && beta0 && alpha0 && psi && workspace && out4, "virnet_elbo_value: NULL pointer");
  if (elbo_geometry("virnet_elbo_value", n, c, cs, cb, h, w)) return 1;
  VIRNET_REQUIRE(eps2 > 0.f, "virnet_elbo_value: eps2 %g must be positive", (double)eps2);
  VIRNET_REQUIRE(aligned4({mu, sigma_est, im_noisy, im_gt, beta0, alpha0, psi, out4}) && ((uintptr_t)workspace & 7) == 0,
                 "virnet_elbo_value: misaligned pointer");
  ElboArgs a{};
  a.mu = mu; a.sigma = sigma_est; a.noisy = im_noisy; a.gt = im_gt; a.beta0 = beta0; a.alpha0 = alpha0; a.psi = psi;
  a.part = static_cast<double*>(workspace);
  a.c = c; a.cs = cs; a.cb = cb; a.hw = (unsigned)(h * w); a.eps2 = eps2; a.with_klig = with_klig != 0;
  const bool vec = a.hw % 4 == 0 && aligned16({mu, sigma_est, im_noisy, im_gt, beta0});
  a.gpp = vec ? a.hw / 4 : a.hw;
  a.items = (unsigned)n * a.gpp;
  const int blocks = elbo_blocks(a.items);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)blocks), block(kThreads);
  dispatch(vec, c, [&] { hipLaunchKernelGGL((elbo_value_kernel<4, 3>), grid, block, 0, s, a); },
           [&] { hipLaunchKernelGGL((elbo_value_kernel<4, 0>), grid, block, 0, s, a); },
           [&] { hipLaunchKernelGGL((elbo_value_kernel<1, 3>), grid, block, 0, s, a); },
           [&] { hipLaunchKernelGGL((elbo_value_kernel<1, 0>), grid, block, 0, s, a); });
  if (int rc = virnet::check_launch("elbo value launch")) return rc;
  const double m = (double)n * c * h * w, mk = (double)n * (cs > cb ? cs : cb) * h * w;
  hipLaunchKernelGGL(elbo_finish_kernel, dim3(1), block, 0, s, a.part, blocks, out4, 1.0 / m, 1.0 / mk);
  return virnet::check_launch("elbo finish launch");
}

extern "C" int virnet_elbo_grad(const float* mu, const float* sigma_est, const float* im_noisy, const float* im_gt, const float* beta0,
                                const float* alpha0, const float* grad_out, float eps2, double w_data, double w_klig, float* dmu, float* dsigma,
                                int n, int c, int cs, int cb, int h, int w, void* stream) {
  VIRNET_REQUIRE(mu && sigma_est && im_noisy && im_gt && beta0 && alpha0 && grad_out && dmu && dsigma, "virnet_elbo_grad: NULL pointer");
  if (elbo_geometry("virnet_elbo_grad", n, c, cs, cb, h, w)) return 1;
  VIRNET_REQUIRE(eps2 > 0.f, "virnet_elbo_grad: eps2 %g must be positive", (double)eps2);
  VIRNET_REQUIRE(aligned4({mu, sigma_est, im_noisy, im_gt, beta0, alpha0, grad_out, dmu, dsigma}), "virnet_elbo_grad: misaligned pointer");
  ElboArgs a{};
  a.mu = mu; a.sigma = sigma_est; a.noisy = im_noisy; a.gt = im_gt; a.beta0 = beta0; a.alpha0 = alpha0; a.gout = grad_out;
  a.dmu = dmu; a.dsigma = dsigma;
  a.c = c; a.cs = cs; a.cb = cb; a.hw = (unsigned)(h * w); a.eps2 = eps2;
  a.wd = w_data / ((double)n * c * h * w);
  a.wk = w_klig / ((double)n * (cs > cb ? cs : cb) * h * w);
  const bool vec = a.hw % 4 == 0 && aligned16({mu, sigma_est, im_noisy, im_gt, beta0, dmu, dsigma});
  a.gpp = vec ? a.hw / 4 : a.hw;
  a.items = (unsigned)n * a.gpp;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)elbo_blocks(a.items)), block(kThreads);
  dispatch(vec, c, [&] { hipLaunchKernelGGL((elbo_grad_kernel<4, 3>), grid, block, 0, s, a); },
           [&] { hipLaunchKernelGGL((elbo_grad_kernel<4, 0>), grid, block, 0, s, a); },
           [&] { hipLaunchKernelGGL((elbo_grad_kernel<1, 3>), grid, block, 0, s, a); },
           [&] { hipLaunchKernelGGL((elbo_grad_kernel<1, 0>), grid, block, 0, s, a); });
  return virnet::check_launch("elbo grad launch");
}

extern "C" int virnet_noise_estimate(const float* im_noisy, const float* im_gt, const double* taps, float* out, int n, int c, int h, int w, int k,
                                     float floor, void* stream) {
  VIRNET_REQUIRE(im_noisy && im_gt && taps && out, "virnet_noise_estimate: NULL pointer");
  VIRNET_REQUIRE(k >= 1 && k <= kNeMaxK && (k & 1), "virnet_noise_estimate: window size %d (odd, 1..%d expected)", k, kNeMaxK);
  VIRNET_REQUIRE(n > 0 && c > 0 && (long long)n * c <= 65535, "virnet_noise_estimate: n=%d c=%d (n*c must be 1..65535)", n, c);
  VIRNET_REQUIRE(h > 0 && w > 0 && h <= (1 << 15) && w <= (1 << 15), "virnet_noise_estimate: image %dx%d outside 1..32768", h, w);
  VIRNET_REQUIRE(k / 2 < (h < w ? h : w), "virnet_noise_estimate: border %d of a %d-tap window does not fit a %dx%d image", k / 2, k, h, w);
  VIRNET_REQUIRE(aligned4({im_noisy, im_gt, out}) && ((uintptr_t)taps & 7) == 0, "virnet_noise_estimate: misaligned pointer");
  NeArgs a;
  a.noisy = im_noisy; a.gt = im_gt; a.taps = taps; a.out = out;
  a.h = h; a.w = w; a.k = k; a.p = k / 2; a.floor = floor;
  a.tiles_x = (w + kNeTx - 1) / kNeTx;
  const int tiles_y = (h + kNeTy - 1) / kNeTy;
  a.rows = kNeTy + 2 * a.p;
  a.pitch = kNeTx + 2 * a.p;
  const size_t lds = (32 + (size_t)a.rows * a.pitch + (size_t)a.rows * kNeTx) * sizeof(double);      // 58.4 KB at k = 31
  VIRNET_REQUIRE(lds <= 65536, "virnet_noise_estimate: %zu bytes of LDS", lds);
  hipLaunchKernelGGL(noise_estimate_kernel, dim3((unsigned)(a.tiles_x * tiles_y), (unsigned)(n * c)), dim3(kThreads), lds,
                     static_cast<hipStream_t>(stream), a);
  return virnet::check_launch("noise estimate launch");
}
