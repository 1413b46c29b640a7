// optim.hip -- gradient-norm clipping and the Adam step on the device (host side: virnet_amd/optim.py; reference train_denoising_syn.py:175-184,
// train_denoising_real.py:172-177, train_SISR.py:224-229: nn.utils.clip_grad_norm_ per sub-network, then torch.optim.Adam.step()).  fp32 tensors.
//
//   The host hands over a LIST of tensors (pointers, sizes, clip set, per-tensor step constants).  The list is cut into chunks of kChunk
//   elements: tensor i owns ceil(numel_i / kChunk) consecutive chunks, chunk ordinals run over the list in order.  A workgroup works on one
//   chunk: thread t owns the four elements at (j * kThreads + t) * 4, j = 0..3, of the chunk -- one 16-byte access each when the tensor's
//   pointers are 16-byte aligned, four 4-byte accesses otherwise (a view at an odd element offset), the same elements either way, so the
//   results do not depend on the alignment.  A chunk that lies wholly inside an aligned tensor takes a form without bounds tests.  The list travels BY VALUE in the kernel arguments, kTable tensors per launch (gradients are new
//   allocations every step: nothing to upload, nothing whose lifetime has to be managed).
//
//   optim_sqnorm_kernel       per chunk: sum of (double)g * (double)g, per thread in element order, wave reduction (shuffles), the block's four
//                             waves through LDS; one fp64 partial to workspace[chunk ordinal].  The host orders the tensors by clip set, so a
//                             set's partials are contiguous.
//   optim_finish_kernel       one workgroup per clip set adds the set's partials in index order (thread t: t, t + 256, ...; then the same tree) and
//                             writes total_norm = (float)sqrt(sum), coef = min(max_norm / (total_norm + 1e-6f), 1) -- the arithmetic of
//                             nn.utils.clip_grad_norm_ (error_if_nonfinite=False); a NaN norm gives a NaN coefficient, an infinite one 0.
//   optim_apply_kernel<MODE>  kAdam: g' = g * coef[set] (g itself for a tensor in no set), then torch's single-tensor Adam in fp32:
//                               g' = fma(weight_decay, p, g')                (only if weight_decay != 0)
//                               m  = fma(g' - m, 1 - beta1, m)
//                               v  = fma((1 - beta2) * g', g', v * beta2)
//                               p  = fma(-step_size, m / (sqrt(v) / bc2_sqrt + eps), p)
//                             with IEEE division and square root; the fused multiply-adds are written out and contraction is off, so both access
//                             forms round alike.  kAdamWriteBack also stores g * coef to the gradient (what the reference's in-place clip
//                             leaves behind).  kScale: g = g * coef[set] only (clip_grad_norm_ for callers that keep another optimizer).
//
// No atomics anywhere: every sum has one fixed order that depends on the list of sizes only, so results are bitwise reproducible.
#include "common.h"
#include "../../include/virnet_hip.h"

#include <cstdint>
#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = VIRNET_OPTIM_CHUNK;      // elements per workgroup: kThreads x 4 x float4
constexpr int kTable = VIRNET_OPTIM_TABLE;      // tensors per launch: the table below is 3.3 KB of the 4 KB of kernel arguments
constexpr int kSets = 16;                       // clip sets per finish launch
constexpr int kPerThread = kChunk / (kThreads * 4);
static_assert(kChunk % (kThreads * 4) == 0, "a thread owns whole float4s");

enum Mode { kAdam = 0, kAdamWriteBack = 1, kScale = 2 };

struct Entry {
  float *p, *g, *m, *v;
  unsigned n;               // elements
  int set;                  // clip set, -1: none
  float step_size, bc2_sqrt;
};

struct Table {
  Entry t[kTable];
  unsigned first[kTable + 1];      // first chunk of tensor i within this launch; first[count] = chunks of the launch
  int count;
  unsigned slot0;                  // chunk ordinal of the launch's first chunk (norm pass: workspace slot)
  const float* coef;               // [sets]
  double* part;
  float w1, beta2, w2, eps, weight_decay;      // 1 - beta1, beta2, 1 - beta2
};
static_assert(sizeof(Table) <= 3584, "the table and the launch's other arguments must stay within 4 KB");

struct FinishArgs {
  unsigned first[kSets], count[kSets];
  float max_norm[kSets];
  const double* part;
  float *total_norm, *coef;      // already offset to the launch's first set
};

// sum over the block in a fixed order: lanes by shuffle tree, then waves 0..3; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// the tensor that owns chunk b of this launch (b < first[count]); uniform over the workgroup
__device__ __forceinline__ int find_entry(const Table& a, unsigned b) {
  int lo = 0, hi = a.count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.first[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

// r[0..cnt) = q[0..cnt), the rest 0; cnt == 4 and vec: one 16-byte access
__device__ __forceinline__ void load4(const float* q, int cnt, bool vec, float (&r)[4]) {
  if (vec && cnt == 4) {
    const float4 t = *reinterpret_cast<const float4*>(q);
    r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = k < cnt ? q[k] : 0.f;
  }
}

__device__ __forceinline__ void store4(float* q, int cnt, bool vec, const float (&r)[4]) {
  if (vec && cnt == 4) {
    *reinterpret_cast<float4*>(q) = make_float4(r[0], r[1], r[2], r[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) q[k] = r[k];
  }
}

__device__ __forceinline__ bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

// FAST: the chunk lies wholly inside a 16-byte aligned tensor -- unconditional 16-byte accesses; otherwise the bounded, per-tensor form.
// Both walk the same elements in the same order through the same arithmetic.
template <bool FAST>
__device__ __forceinline__ double sqnorm_chunk(const float* g, unsigned n, unsigned off, bool vec) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const unsigned i = off + (unsigned)(j * kThreads + threadIdx.x) * 4u;
    if (!FAST && i >= n) break;
    const int cnt = FAST ? 4 : (n - i < 4u ? (int)(n - i) : 4);
    float x[4];
    load4(g + i, cnt, FAST || vec, x);
#pragma unroll
    for (int k = 0; k < 4; ++k) s += (double)x[k] * (double)x[k];
  }
  return s;
}

__global__ __launch_bounds__(kThreads) void optim_sqnorm_kernel(const Table a) {
  __shared__ double red[kThreads / 64];
  const unsigned b = blockIdx.x;
  const int e = find_entry(a, b);
  const float* const g = a.t[e].g;
  const unsigned n = a.t[e].n;
  const unsigned off = (b - a.first[e]) * (unsigned)kChunk;
  const bool vec = aligned16(g);
  double s = (vec && n - off >= (unsigned)kChunk) ? sqnorm_chunk<true>(g, n, off, vec) : sqnorm_chunk<false>(g, n, off, vec);
  s = block_sum(s, red);
  if (threadIdx.x == 0) a.part[a.slot0 + b] = s;
}

__global__ __launch_bounds__(kThreads) void optim_finish_kernel(const FinishArgs a) {
  __shared__ double red[kThreads / 64];
  const int set = blockIdx.x;
  const double* const part = a.part + a.first[set];
  const unsigned count = a.count[set];
  double s = 0.0;
  for (unsigned i = threadIdx.x; i < count; i += kThreads) s += part[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(s);
    const float c = a.max_norm[set] / (norm + 1e-6f);
    a.total_norm[set] = norm;
    a.coef[set] = c > 1.f ? 1.f : c;      // (a NaN stays a NaN, as through torch.clamp)
  }
}

struct Consts {
  float coef, step_size, bc2_sqrt, w1, beta2, w2, eps, wd;
  bool clip;
};

template <int MODE, bool FAST>
__device__ __forceinline__ void apply_chunk(float* p, float* g, float* m, float* v, unsigned n, unsigned off, bool vec, const Consts& c) {
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const unsigned i = off + (unsigned)(j * kThreads + threadIdx.x) * 4u;
    if (!FAST && i >= n) break;
    const int cnt = FAST ? 4 : (n - i < 4u ? (int)(n - i) : 4);
    const bool wide = FAST || vec;
    float gg[4];
    load4(g + i, cnt, wide, gg);
    if (c.clip) {
#pragma unroll
      for (int k = 0; k < 4; ++k) gg[k] = gg[k] * c.coef;
    }
    if (MODE == kScale) {
      store4(g + i, cnt, wide, gg);
      continue;
    }
    if (MODE == kAdamWriteBack && c.clip) store4(g + i, cnt, wide, gg);
    float pp[4], mm[4], vv[4];
    load4(p + i, cnt, wide, pp);
    load4(m + i, cnt, wide, mm);
    load4(v + i, cnt, wide, vv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float q = gg[k];
      if (c.wd != 0.f) q = fmaf(c.wd, pp[k], q);
      mm[k] = fmaf(q - mm[k], c.w1, mm[k]);
      vv[k] = fmaf(c.w2 * q, q, vv[k] * c.beta2);
      const float denom = sqrtf(vv[k]) / c.bc2_sqrt + c.eps;
      pp[k] = fmaf(-c.step_size, mm[k] / denom, pp[k]);
    }
    store4(m + i, cnt, wide, mm);
    store4(v + i, cnt, wide, vv);
    store4(p + i, cnt, wide, pp);
  }
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void optim_apply_kernel(const Table a) {
  const unsigned b = blockIdx.x;
  const int e = find_entry(a, b);
  const int set = a.t[e].set;
  if (MODE == kScale && set < 0) return;
  float* const g = a.t[e].g;
  float* const p = a.t[e].p;
  float* const m = a.t[e].m;
  float* const v = a.t[e].v;
  const unsigned n = a.t[e].n;
  const unsigned off = (b - a.first[e]) * (unsigned)kChunk;
  const bool vec = MODE == kScale ? aligned16(g) : aligned16(g, p, m, v);
  Consts c;
  c.clip = set >= 0;
  c.coef = c.clip ? a.coef[set] : 1.f;
  c.step_size = a.t[e].step_size; c.bc2_sqrt = a.t[e].bc2_sqrt;
  c.w1 = a.w1; c.beta2 = a.beta2; c.w2 = a.w2; c.eps = a.eps; c.wd = a.weight_decay;
  if (vec && n - off >= (unsigned)kChunk)
    apply_chunk<MODE, true>(p, g, m, v, n, off, vec, c);
  else
    apply_chunk<MODE, false>(p, g, m, v, n, off, vec, c);
}

// ---- host: the plan ---------------------------------------------------------------------------------------------------------------------
long long chunks_of(long long numel) { return (numel + kChunk - 1) / kChunk; }

// 0 when the list is one the kernels take (error slot set otherwise)
int check_list(const char* who, const long long* numel, const int* set, int count, int nsets) {
  VIRNET_REQUIRE(count >= 0 && nsets >= 0 && (count == 0 || (numel && set)), "%s: bad list (count %d, sets %d)", who, count, nsets);
  long long total = 0;
  for (int i = 0; i < count; ++i) {
    VIRNET_REQUIRE(numel[i] >= 1 && numel[i] < (1ll << 31), "%s: tensor %d has %lld elements (1 .. 2^31 - 1 expected)", who, i, numel[i]);
    VIRNET_REQUIRE(set[i] >= -1 && set[i] < nsets, "%s: tensor %d is in clip set %d (-1 .. %d expected)", who, i, set[i], nsets - 1);
    if (i > 0) {
      const bool ordered = set[i] < 0 ? true : (set[i - 1] >= 0 && set[i - 1] <= set[i]);
      VIRNET_REQUIRE(ordered, "%s: tensor %d (clip set %d) follows clip set %d: the list must be ordered by set, tensors in no set last", who, i,
                     set[i], set[i - 1]);
    }
    total += chunks_of(numel[i]);
  }
  VIRNET_REQUIRE(total < (1ll << 31), "%s: %lld chunks (below 2^31 expected)", who, total);
  return 0;
}

// The layout of a checked list, the one every entry below launches from (virnet_optim_plan hands it out as it is): chunk ordinals run over
// the list in order, launch t carries tensors [t * kTable, (t + 1) * kTable), a set's chunks are one range of ordinals.
struct Plan {
  std::vector<int> first_chunk, table, set_first, set_chunks;      // [count + 1] (the last: chunks in all), [count], [nsets], [nsets]
};

Plan make_plan(const long long* numel, const int* set, int count, int nsets) {
  Plan pl;
  pl.first_chunk.resize(count + 1);
  pl.table.resize(count);
  pl.set_first.assign(nsets, 0);
  pl.set_chunks.assign(nsets, 0);
  long long c = 0;
  for (int i = 0; i < count; ++i) {
    pl.first_chunk[i] = (int)c;
    pl.table[i] = i / kTable;
    if (set[i] >= 0 && set[i] < nsets) {
      if (pl.set_chunks[set[i]] == 0) pl.set_first[set[i]] = (int)c;
      pl.set_chunks[set[i]] += (int)chunks_of(numel[i]);
    }
    c += chunks_of(numel[i]);
  }
  pl.first_chunk[count] = (int)c;
  return pl;
}

struct List {
  void* const* p; void* const* g; void* const* m; void* const* v;
  const long long* numel; const int* set; const float* step_size; const float* bc2_sqrt;
};

// tensors [i0, i0 + count) of the plan -- one of its tables -- as a launch's arguments
void fill(Table& a, const List& l, const Plan& pl, int i0, int count) {
  a.count = count;
  a.slot0 = (unsigned)pl.first_chunk[i0];
  for (int i = 0; i < count; ++i) {
    Entry& t = a.t[i];
    const int s = i0 + i;
    t.p = l.p ? static_cast<float*>(l.p[s]) : nullptr;
    t.g = static_cast<float*>(l.g[s]);
    t.m = l.m ? static_cast<float*>(l.m[s]) : nullptr;
    t.v = l.v ? static_cast<float*>(l.v[s]) : nullptr;
    t.n = (unsigned)l.numel[s];
    t.set = l.set[s];
    t.step_size = l.step_size ? l.step_size[s] : 0.f;
    t.bc2_sqrt = l.bc2_sqrt ? l.bc2_sqrt[s] : 1.f;
    a.first[i] = (unsigned)(pl.first_chunk[s] - pl.first_chunk[i0]);
  }
  a.first[count] = (unsigned)(pl.first_chunk[i0 + count] - pl.first_chunk[i0]);
}

// [i0, i1): the tensors of the table that begins at i0
int table_end(const Plan& pl, int i0, int count) {
  int i1 = i0;
  while (i1 < count && pl.table[i1] == pl.table[i0]) ++i1;
  return i1;
}

int check_pointers(const char* who, void* const* q, int count, const char* what) {
  VIRNET_REQUIRE(q, "%s: NULL list of %s pointers", who, what);
  for (int i = 0; i < count; ++i) VIRNET_REQUIRE(q[i] && ((uintptr_t)q[i] & 3) == 0, "%s: %s pointer of tensor %d is NULL or misaligned", who, what, i);
  return 0;
}

template <int MODE>
int launch_apply(const char* who, const List& l, int count, const float* coef, float w1, float beta2, float w2, float eps, float weight_decay,
                 hipStream_t s) {
  Table a{};
  a.coef = coef;
  a.w1 = w1; a.beta2 = beta2; a.w2 = w2; a.eps = eps; a.weight_decay = weight_decay;
  const Plan pl = make_plan(l.numel, l.set, count, 0);
  for (int i0 = 0; i0 < count;) {
    const int i1 = table_end(pl, i0, count);
    if (MODE == kScale && l.set[i0] < 0) break;      // tensors in no set come last: nothing left to scale
    fill(a, l, pl, i0, i1 - i0);
    hipLaunchKernelGGL((optim_apply_kernel<MODE>), dim3(a.first[i1 - i0]), dim3(kThreads), 0, s, a);
    if (int rc = virnet::check_launch(who)) return rc;
    i0 = i1;
  }
  return 0;
}

}  // namespace

extern "C" int virnet_optim_plan(const long long* numel, const int* set, int count, int nsets, int* first_chunk, int* table, int* set_first,
                                 int* set_chunks) {
  if (check_list("virnet_optim_plan", numel, set, count, nsets)) return 1;
  VIRNET_REQUIRE((count == 0 || (first_chunk && table)) && (nsets == 0 || (set_first && set_chunks)), "virnet_optim_plan: NULL output");
  const Plan pl = make_plan(numel, set, count, nsets);
  for (int i = 0; i < count; ++i) {
    first_chunk[i] = pl.first_chunk[i];
    table[i] = pl.table[i];
  }
  for (int s = 0; s < nsets; ++s) {
    set_first[s] = pl.set_first[s];
    set_chunks[s] = pl.set_chunks[s];
  }
  return 0;
}

extern "C" size_t virnet_optim_workspace_bytes(const long long* numel, const int* set, int count) {
  long long c = 0;
  for (int i = 0; i < count; ++i) {
    if (numel[i] < 1 || numel[i] >= (1ll << 31)) {
      virnet::set_error("virnet_optim_workspace_bytes: tensor %d has %lld elements (1 .. 2^31 - 1 expected)", i, numel[i]);
      return 0;
    }
    if (set[i] >= 0) c += chunks_of(numel[i]);
  }
  return (size_t)(c > 0 ? c : 1) * sizeof(double);
}

extern "C" int virnet_optim_grad_norms(void* const* g, const long long* numel, const int* set, int count, const float* max_norm, int nsets,
                                       void* workspace, float* total_norm, float* coef, void* stream) {
  const char* const who = "virnet_optim_grad_norms";
  if (check_list(who, numel, set, count, nsets)) return 1;
  VIRNET_REQUIRE(nsets >= 1 && max_norm && workspace && total_norm && coef, "%s: NULL pointer or no clip set", who);
  VIRNET_REQUIRE(((uintptr_t)workspace & 7) == 0 && (((uintptr_t)total_norm | (uintptr_t)coef) & 3) == 0, "%s: misaligned pointer", who);
  if (check_pointers(who, g, count, "gradient")) return 1;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int in_sets = 0;
  while (in_sets < count && set[in_sets] >= 0) ++in_sets;
  const List l{nullptr, g, nullptr, nullptr, numel, set, nullptr, nullptr};
  Table a{};
  a.part = static_cast<double*>(workspace);
  FinishArgs f{};
  const Plan pl = make_plan(numel, set, count, nsets);
  for (int i0 = 0; i0 < in_sets;) {
    int i1 = table_end(pl, i0, count);
    if (i1 > in_sets) i1 = in_sets;                  // (tensors in no set have no partials)
    fill(a, l, pl, i0, i1 - i0);
    hipLaunchKernelGGL(optim_sqnorm_kernel, dim3(a.first[i1 - i0]), dim3(kThreads), 0, s, a);
    if (int rc = virnet::check_launch("optim sqnorm launch")) return rc;
    i0 = i1;
  }
  f.part = static_cast<const double*>(workspace);
  for (int s0 = 0; s0 < nsets; s0 += kSets) {
    const int ns = nsets - s0 < kSets ? nsets - s0 : kSets;
    for (int k = 0; k < ns; ++k) {
      f.first[k] = (unsigned)pl.set_first[s0 + k];
      f.count[k] = (unsigned)pl.set_chunks[s0 + k];
      f.max_norm[k] = max_norm[s0 + k];
    }
    f.total_norm = total_norm + s0;
    f.coef = coef + s0;
    hipLaunchKernelGGL(optim_finish_kernel, dim3((unsigned)ns), dim3(kThreads), 0, s, f);
    if (int rc = virnet::check_launch("optim finish launch")) return rc;
  }
  return 0;
}

extern "C" int virnet_optim_adam_step(void* const* p, void* const* g, void* const* m, void* const* v, const long long* numel, const int* set,
                                      const float* step_size, const float* bc2_sqrt, int count, int nsets, const float* coef, float one_minus_beta1,
                                      float beta2, float one_minus_beta2, float eps, float weight_decay, int write_back, void* stream) {
  const char* const who = "virnet_optim_adam_step";
  if (check_list(who, numel, set, count, nsets)) return 1;
  VIRNET_REQUIRE(step_size && bc2_sqrt, "%s: NULL step constants", who);
  VIRNET_REQUIRE(nsets == 0 || (coef && ((uintptr_t)coef & 3) == 0), "%s: NULL or misaligned coefficient pointer", who);
  if (check_pointers(who, p, count, "parameter") || check_pointers(who, g, count, "gradient") || check_pointers(who, m, count, "exp_avg") ||
      check_pointers(who, v, count, "exp_avg_sq"))
    return 1;
  for (int i = 0; i < count; ++i)
    VIRNET_REQUIRE(bc2_sqrt[i] > 0.f, "%s: tensor %d has bias correction %g (positive expected: step >= 1, beta2 < 1)", who, i, (double)bc2_sqrt[i]);
  const List l{p, g, m, v, numel, set, step_size, bc2_sqrt};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (write_back)
    return launch_apply<kAdamWriteBack>("optim apply launch", l, count, coef, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay, s);
  return launch_apply<kAdam>("optim apply launch", l, count, coef, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay, s);
}

extern "C" int virnet_optim_scale_grads(void* const* g, const long long* numel, const int* set, int count, int nsets, const float* coef,
                                        void* stream) {
  const char* const who = "virnet_optim_scale_grads";
  if (check_list(who, numel, set, count, nsets)) return 1;
  VIRNET_REQUIRE(nsets == 0 || (coef && ((uintptr_t)coef & 3) == 0), "%s: NULL or misaligned coefficient pointer", who);
  if (check_pointers(who, g, count, "gradient")) return 1;
  const List l{nullptr, g, nullptr, nullptr, numel, set, nullptr, nullptr};
  return launch_apply<kScale>("optim scale launch", l, count, coef, 0.f, 0.f, 0.f, 0.f, 0.f, static_cast<hipStream_t>(stream));
}
