// gradsync.hip -- the gradient buckets of data-parallel training on the device (host side: virnet_amd/dist.py; what DistributedDataParallel's
// reducer does around train_denoising_syn.py:71, train_denoising_real.py:70 and train_SISR.py:95: gradients into flat buckets before the
// all-reduce, bucket slices back into gradients after it).  fp32 tensors.
//
//   pack      count tensors -> one flat bucket at given element offsets, every element times `scale` (one fp32 rounding: the bits of
//             bucket[off:off+n].copy_(g).mul_(scale)); a NULL tensor writes zeros to its slot; words outside every slot are not touched.
//   unpack    bucket slices -> count tensors, every element times `scale` or, when given, times the float at a device pointer (the fused
//             backward's power-of-two un-scale lives on the device) -- the bits of bucket[off:off+n].clone().mul_(s).
//
//   Both are ONE kernel: a list of (source, destination, elements) ranges, destination = source * factor.  As in optim.hip the list travels BY
//   VALUE in the kernel arguments, kTable ranges per launch (a further launch when the table is full), and is cut into chunks of kChunk
//   elements, one workgroup each, so that a 1-element bias and an 82 944-element weight load the grid evenly.  Bucket offsets are arbitrary
//   (slots lie in production order), so a range's two ends have independent alignments: the chunks of a range are laid over the DESTINATION's
//   16-byte grid (the range starts `s` = 0..3 elements into its first quad), a quad that lies wholly inside the range is stored with one
//   16-byte access and loaded with one when the source shares the phase (four 4-byte loads otherwise); the quads cut by the range's ends are
//   the scalar head and tail.  Every element goes through the same single multiply, so the bits do not depend on the alignment.
//
// No atomics, no scratch, no workspace, nothing that synchronises with the host: both entries can be captured.
#include "common.h"
#include "../../include/virnet_hip.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = VIRNET_GRADSYNC_CHUNK;      // elements of the destination's 16-byte grid per workgroup: kThreads x 4 x float4
constexpr int kTable = VIRNET_GRADSYNC_TABLE;      // ranges per launch: 3 KB of the 4 KB of kernel arguments
constexpr int kPerThread = kChunk / (kThreads * 4);
static_assert(kChunk % (kThreads * 4) == 0, "a thread owns whole float4s");

struct Range {
  const float* src;      // NULL: zeros
  float* dst;
  unsigned n;            // elements, >= 1
  unsigned first;        // first chunk of the range within this launch
};

struct Table {
  Range t[kTable];
  unsigned chunks;       // of the launch
  int count;
  float scale;
  const float* scale_dev;      // not NULL: the factor is read from here
};
static_assert(sizeof(Range) == 24, "a range is three 8-byte words");
static_assert(sizeof(Table) <= 3584, "the table must stay within the 4 KB of kernel arguments");

// the range that owns chunk b of this launch (b < chunks); uniform over the workgroup
__device__ __forceinline__ int find_range(const Table& a, unsigned b) {
  int lo = 0, hi = a.count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.t[mid].first <= b) lo = mid; else hi = mid;
  }
  return lo;
}

// elements of the destination's 16-byte grid before the range's first one
__host__ __device__ __forceinline__ unsigned phase(const void* p) { return (unsigned)(((uintptr_t)p >> 2) & 3u); }

// FULL: every quad of the chunk lies inside the range -- no bounds tests.  WIDE: the source shares the destination's phase.
template <bool FULL>
__device__ __forceinline__ void copy_chunk(const float* src, float* dst, unsigned s, unsigned n, unsigned j0, bool wide, float f) {
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const unsigned j = j0 + (unsigned)(k * kThreads + threadIdx.x) * 4u;      // grid position of the quad; element i = j - s
    if (!FULL && j >= s + n) break;
    if (FULL || (j >= s && j + 4u <= s + n)) {
      const unsigned i = j - s;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (src) {
        if (wide) {
          v = *reinterpret_cast<const float4*>(src + i);
        } else {
          v.x = src[i]; v.y = src[i + 1]; v.z = src[i + 2]; v.w = src[i + 3];
        }
        v.x = v.x * f; v.y = v.y * f; v.z = v.z * f; v.w = v.w * f;
      }
      *reinterpret_cast<float4*>(dst + i) = v;
    } else {
#pragma unroll
      for (unsigned e = 0; e < 4u; ++e) {
        const unsigned q = j + e;
        if (q >= s && q < s + n) dst[q - s] = src ? src[q - s] * f : 0.f;
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void gradsync_copy_kernel(const Table a) {
  const unsigned b = blockIdx.x;
  const int e = find_range(a, b);
  const float* const src = a.t[e].src;
  float* const dst = a.t[e].dst;
  const unsigned n = a.t[e].n;
  const unsigned s = phase(dst);
  const unsigned j0 = (b - a.t[e].first) * (unsigned)kChunk;
  const bool wide = src && phase(src) == s && (((uintptr_t)src | (uintptr_t)dst) & 3) == 0;
  const float f = a.scale_dev ? *a.scale_dev : a.scale;
  if (j0 >= s && j0 + (unsigned)kChunk <= s + n)
    copy_chunk<true>(src, dst, s, n, j0, wide, f);
  else
    copy_chunk<false>(src, dst, s, n, j0, wide, f);
}

long long chunks_of(const void* dst, long long numel) { return ((long long)phase(dst) + numel + kChunk - 1) / kChunk; }

struct Item {
  const float* src;
  float* dst;
  long long n;
};

// Launches `count` checked ranges through the table, kTable at a time.  `at(i)` yields range i (n == 0: skipped).
template <class At>
int launch(const char* who, int count, At at, float scale, const float* scale_dev, hipStream_t s) {
  Table a{};
  a.scale = scale;
  a.scale_dev = scale_dev;
  long long chunks = 0;
  int k = 0;
  for (int i = 0; i <= count; ++i) {
    if (i < count) {
      const Item it = at(i);
      if (it.n == 0) continue;
      a.t[k] = Range{it.src, it.dst, (unsigned)it.n, (unsigned)chunks};
      chunks += chunks_of(it.dst, it.n);
      ++k;
    }
    if (k == kTable || (i == count && k > 0) || chunks >= (1ll << 30)) {
      a.count = k;
      a.chunks = (unsigned)chunks;
      hipLaunchKernelGGL(gradsync_copy_kernel, dim3(a.chunks), dim3(kThreads), 0, s, a);
      if (int rc = virnet::check_launch(who)) return rc;
      k = 0;
      chunks = 0;
    }
  }
  return 0;
}

int check_slots(const char* who, const long long* numel, const long long* offset, int count, long long bucket_numel) {
  VIRNET_REQUIRE(count >= 0 && (count == 0 || (numel && offset)), "%s: bad list (count %d)", who, count);
  VIRNET_REQUIRE(bucket_numel >= 0, "%s: bucket of %lld elements", who, bucket_numel);
  for (int i = 0; i < count; ++i) {
    VIRNET_REQUIRE(numel[i] >= 0 && numel[i] < (1ll << 31), "%s: tensor %d has %lld elements (0 .. 2^31 - 1 expected)", who, i, numel[i]);
    VIRNET_REQUIRE(offset[i] >= 0 && offset[i] <= bucket_numel && numel[i] <= bucket_numel - offset[i],
                   "%s: slot %d = [%lld, %lld) lies beyond the bucket's %lld elements", who, i, offset[i], offset[i] + numel[i], bucket_numel);
  }
  return 0;
}

}  // namespace

extern "C" int virnet_gradsync_launches(const long long* numel, int count) {
  int live = 0;
  for (int i = 0; i < count; ++i)
    if (numel && numel[i] > 0) ++live;
  return (live + kTable - 1) / kTable;
}

extern "C" int virnet_gradsync_pack(void* const* src, const long long* numel, const long long* offset, int count, float* bucket,
                                    long long bucket_numel, float scale, void* stream) {
  const char* const who = "virnet_gradsync_pack";
  if (check_slots(who, numel, offset, count, bucket_numel)) return 1;
  VIRNET_REQUIRE(count == 0 || (src && bucket && ((uintptr_t)bucket & 3) == 0), "%s: NULL or misaligned pointer", who);
  for (int i = 0; i < count; ++i) VIRNET_REQUIRE(((uintptr_t)src[i] & 3) == 0, "%s: pointer of tensor %d is misaligned", who, i);
  return launch("gradsync pack launch", count,
                [&](int i) { return Item{static_cast<const float*>(src[i]), bucket + offset[i], numel[i]}; }, scale, nullptr,
                static_cast<hipStream_t>(stream));
}

extern "C" int virnet_gradsync_unpack(const float* bucket, long long bucket_numel, const long long* offset, const long long* numel,
                                      void* const* dst, int count, float scale, const float* scale_dev, void* stream) {
  const char* const who = "virnet_gradsync_unpack";
  if (check_slots(who, numel, offset, count, bucket_numel)) return 1;
  VIRNET_REQUIRE(count == 0 || (dst && bucket && ((uintptr_t)bucket & 3) == 0), "%s: NULL or misaligned pointer", who);
  VIRNET_REQUIRE(((uintptr_t)scale_dev & 3) == 0, "%s: misaligned factor pointer", who);
  for (int i = 0; i < count; ++i)
    VIRNET_REQUIRE(numel[i] == 0 || (dst[i] && ((uintptr_t)dst[i] & 3) == 0), "%s: pointer of tensor %d is NULL or misaligned", who, i);
  return launch("gradsync unpack launch", count,
                [&](int i) { return Item{bucket + offset[i], static_cast<float*>(dst[i]), numel[i]}; }, scale, scale_dev,
                static_cast<hipStream_t>(stream));
}
