// ema.hip -- exponential moving average of the weights on the device (host side: virnet_amd/ema.py).  fp32 tensors.
//
//   The host hands over a LIST of tensor pairs (two pointers and a size each), in the idiom of optim.hip: the list is cut into chunks of
//   kChunk elements, tensor i owns ceil(numel_i / kChunk) consecutive chunks, a workgroup works on one chunk, thread t owns the four
//   elements at (j * kThreads + t) * 4, j = 0..3, of the chunk -- one 16-byte access each when BOTH pointers of the pair are 16-byte
//   aligned, four 4-byte accesses otherwise (a view at an odd element offset), the same elements either way.  A chunk that lies wholly
//   inside an aligned pair takes a form without bounds tests.  The list travels BY VALUE in the kernel arguments, kTable pairs per launch:
//   no host-to-device copy, no synchronisation, no workspace.
//
//   ema_kernel<kUpdate>   e = e + w * (p - e) as three fp32 operations, each rounded on its own (contraction is switched off for
//                         the unit: no fused multiply-add).  This is the form whose fixpoint is exact: p == e gives
//                         d = +0, t = +0 and e + 0 = e, bit for bit (w is finite and non-negative; a -0 becomes +0).  p is read only.
//   ema_kernel<kSwap>     exchanges the two tensors word by word: the values never pass through a floating-point operation, so NaN
//                         payloads and signed zeros move as they are.
//
// No atomics, no LDS, no scratch: plain vector loads and stores, every element touched by exactly one thread.
#include "common.h"
#include "../../include/virnet_hip.h"

#include <cstdint>

// The update is written with plain operators under this pragma, as optim.hip's arithmetic is.  (__fmul_rn / __fadd_rn do not keep the two
// apart: they are inline functions of a header compiled with contraction allowed, and once inlined the compiler fuses them into one fma.)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = VIRNET_OPTIM_CHUNK;      // elements per workgroup: kThreads x 4 x four words
constexpr int kTable = VIRNET_OPTIM_TABLE;      // pairs per launch: the table below is 1.8 KB of the 4 KB of kernel arguments
constexpr int kPerThread = kChunk / (kThreads * 4);
static_assert(kChunk % (kThreads * 4) == 0, "a thread owns whole 16-byte groups");

enum Mode { kUpdate = 0, kSwap = 1 };

struct Entry {
  unsigned *a, *b;          // update: a = e (read and written), b = p (read); swap: both read and written
  unsigned n;               // elements
};

struct Table {
  Entry t[kTable];
  unsigned first[kTable + 1];      // first chunk of pair i within this launch; first[count] = chunks of the launch
  int count;
  float w;
};
static_assert(sizeof(Table) <= 3584, "the table must stay within the 4 KB of kernel arguments");

// the pair that owns chunk b of this launch (b < first[count]); uniform over the workgroup
__device__ __forceinline__ int find_entry(const Table& a, unsigned b) {
  int lo = 0, hi = a.count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.first[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

// r[0..cnt) = q[0..cnt), the rest 0; cnt == 4 and vec: one 16-byte access
__device__ __forceinline__ void load4(const unsigned* q, int cnt, bool vec, unsigned (&r)[4]) {
  if (vec && cnt == 4) {
    const uint4 t = *reinterpret_cast<const uint4*>(q);
    r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = k < cnt ? q[k] : 0u;
  }
}

__device__ __forceinline__ void store4(unsigned* q, int cnt, bool vec, const unsigned (&r)[4]) {
  if (vec && cnt == 4) {
    *reinterpret_cast<uint4*>(q) = make_uint4(r[0], r[1], r[2], r[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) q[k] = r[k];
  }
}

// FAST: the chunk lies wholly inside a 16-byte aligned pair -- unconditional 16-byte accesses; otherwise the bounded, per-pair form.
// Both walk the same elements through the same arithmetic.
template <int MODE, bool FAST>
__device__ __forceinline__ void chunk(unsigned* a, unsigned* b, unsigned n, unsigned off, bool vec, float w) {
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const unsigned i = off + (unsigned)(j * kThreads + threadIdx.x) * 4u;
    if (!FAST && i >= n) break;
    const int cnt = FAST ? 4 : (n - i < 4u ? (int)(n - i) : 4);
    const bool wide = FAST || vec;
    unsigned x[4], y[4];
    load4(a + i, cnt, wide, x);
    load4(b + i, cnt, wide, y);
    if (MODE == kSwap) {
      store4(a + i, cnt, wide, y);
      store4(b + i, cnt, wide, x);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float e = __uint_as_float(x[k]);
        const float d = __uint_as_float(y[k]) - e;
        const float t = w * d;
        x[k] = __float_as_uint(e + t);
      }
      store4(a + i, cnt, wide, x);
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void ema_kernel(const Table t) {
  const unsigned blk = blockIdx.x;
  const int e = find_entry(t, blk);
  unsigned* const a = t.t[e].a;
  unsigned* const b = t.t[e].b;
  const unsigned n = t.t[e].n;
  const unsigned off = (blk - t.first[e]) * (unsigned)kChunk;
  const bool vec = ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0;
  if (vec && n - off >= (unsigned)kChunk)
    chunk<MODE, true>(a, b, n, off, vec, t.w);
  else
    chunk<MODE, false>(a, b, n, off, vec, t.w);
}

long long chunks_of(long long numel) { return (numel + kChunk - 1) / kChunk; }

// 0 when the list is one the kernels take (error slot set otherwise)
int check_list(const char* who, void* const* a, void* const* b, const long long* numel, int count) {
  VIRNET_REQUIRE(a && b && numel, "%s: NULL list", who);
  long long total = 0;
  for (int i = 0; i < count; ++i) {
    VIRNET_REQUIRE(numel[i] >= 1 && numel[i] < (1ll << 31), "%s: tensor %d has %lld elements (1 .. 2^31 - 1 expected)", who, i, numel[i]);
    VIRNET_REQUIRE(a[i] && b[i] && ((((uintptr_t)a[i]) | ((uintptr_t)b[i])) & 3) == 0, "%s: a pointer of tensor %d is NULL or misaligned", who, i);
    VIRNET_REQUIRE(a[i] != b[i], "%s: the two pointers of tensor %d are the same", who, i);
    total += chunks_of(numel[i]);
  }
  VIRNET_REQUIRE(total < (1ll << 31), "%s: %lld chunks (below 2^31 expected)", who, total);
  return 0;
}

template <int MODE>
int launch(const char* who, void* const* a, void* const* b, const long long* numel, int count, float w, hipStream_t s) {
  Table t{};
  t.w = w;
  for (int i0 = 0; i0 < count; i0 += kTable) {
    const int n = count - i0 < kTable ? count - i0 : kTable;
    unsigned c = 0;
    for (int i = 0; i < n; ++i) {
      t.t[i].a = static_cast<unsigned*>(a[i0 + i]);
      t.t[i].b = static_cast<unsigned*>(b[i0 + i]);
      t.t[i].n = (unsigned)numel[i0 + i];
      t.first[i] = c;
      c += (unsigned)chunks_of(numel[i0 + i]);
    }
    t.first[n] = c;
    t.count = n;
    hipLaunchKernelGGL((ema_kernel<MODE>), dim3(c), dim3(kThreads), 0, s, t);
    if (int rc = virnet::check_launch(who)) return rc;
  }
  return 0;
}

}  // namespace

extern "C" int virnet_ema_update(void* const* e, void* const* p, const long long* numel, int count, float w, void* stream) {
  const char* const who = "virnet_ema_update";
  VIRNET_REQUIRE(count >= 0, "%s: bad list (count %d)", who, count);
  if (count == 0) return 0;
  VIRNET_REQUIRE(w >= 0.f && w <= 1.f, "%s: weight %g (0 .. 1 expected)", who, (double)w);
  if (check_list(who, e, p, numel, count)) return 1;
  return launch<kUpdate>("ema update launch", e, p, numel, count, w, static_cast<hipStream_t>(stream));
}

extern "C" int virnet_ema_swap(void* const* a, void* const* b, const long long* numel, int count, void* stream) {
  const char* const who = "virnet_ema_swap";
  VIRNET_REQUIRE(count >= 0, "%s: bad list (count %d)", who, count);
  if (count == 0) return 0;
  if (check_list(who, a, b, numel, count)) return 1;
  return launch<kSwap>("ema swap launch", a, b, numel, count, 0.f, static_cast<hipStream_t>(stream));
}
