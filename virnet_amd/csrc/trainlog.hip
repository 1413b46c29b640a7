// trainlog.hip -- the per-step scalars of a training loop kept on the device (host side: virnet_amd/trainlog.py; reference
// train_denoising_syn.py:186-198: four .item() calls and two norm reads on every step, which stall the host once per step).
//
//   The log is one device buffer: k fp64 running sums, then a ring of `capacity` rows of k fp32 values.  A step's scalars live wherever the
//   step left them (the loss and its three parts, the optimizer's norm vector): their device pointers travel by value in the kernel
//   arguments, as the optimizer's tensor table does (optim.hip), so a push is one launch with no host-to-device copy and no synchronisation.
//
//   trainlog_push_kernel         one workgroup, one thread per value: row[slot][t] = x_t; sums[t] += double(x_t) / double(num_iter).  The
//                                pushes of a stream run in step order, each thread owns its sum, and the fp64 division and addition are
//                                IEEE operations: the sum is bit for bit the Python double of `acc += x.item() / num_iter` step by step.
//   trainlog_reset_kernel        sums[t] = 0.
//
// No atomics, no scratch, no LDS.
#include "common.h"
#include "../../include/virnet_hip.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int kMax = VIRNET_TRAINLOG_MAX;
constexpr int kThreads = 64;

struct PushArgs {
  const float* src[kMax];        // source s holds count[s] consecutive fp32 values
  int first[kMax + 1];           // value ordinal of source s's first value; first[nsrc] = k
  int nsrc, k, num_iter;
  double* sums;                  // [k]
  float* row;                    // the ring's row of this step, [k]
};

__global__ __launch_bounds__(kThreads) void trainlog_push_kernel(const PushArgs a) {
  const int t = threadIdx.x;
  if (t >= a.k) return;
  int s = 0;
#pragma unroll
  for (int j = 1; j < kMax; ++j)
    if (j < a.nsrc && t >= a.first[j]) s = j;
  // (a select chain over the by-value table, not a dynamic index into it: the table stays in scalar registers, nothing goes to scratch)
  const float* p = a.src[0];
  int base = a.first[0];
#pragma unroll
  for (int j = 1; j < kMax; ++j)
    if (s == j) { p = a.src[j]; base = a.first[j]; }
  const float x = p[t - base];
  a.row[t] = x;
  a.sums[t] = a.sums[t] + (double)x / (double)a.num_iter;
}

__global__ __launch_bounds__(kThreads) void trainlog_reset_kernel(double* sums, int k) {
  if ((int)threadIdx.x < k) sums[threadIdx.x] = 0.0;
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" size_t virnet_trainlog_bytes(int k, int capacity) {
  if (k < 1 || k > kMax || capacity < 1 || capacity > VIRNET_TRAINLOG_MAX_CAPACITY) {
    virnet::set_error("virnet_trainlog_bytes: k %d (1 .. %d), capacity %d (1 .. %d)", k, kMax, capacity, VIRNET_TRAINLOG_MAX_CAPACITY);
    return 0;
  }
  return (size_t)k * 8 + (size_t)capacity * (size_t)k * 4;
}

extern "C" int virnet_trainlog_push(const void* const* src, const int* count, int nsrc, void* log, int k, int capacity, int slot, int num_iter,
                                    void* stream) {
  const char* const who = "virnet_trainlog_push";
  VIRNET_REQUIRE(k >= 1 && k <= kMax, "%s: %d values (1 .. %d expected)", who, k, kMax);
  VIRNET_REQUIRE(capacity >= 1 && capacity <= VIRNET_TRAINLOG_MAX_CAPACITY, "%s: capacity %d (1 .. %d expected)", who, capacity,
                 VIRNET_TRAINLOG_MAX_CAPACITY);
  VIRNET_REQUIRE(slot >= 0 && slot < capacity, "%s: slot %d outside the ring of %d rows", who, slot, capacity);
  VIRNET_REQUIRE(num_iter >= 1, "%s: num_iter %d (a positive step count expected)", who, num_iter);
  VIRNET_REQUIRE(src && count && log, "%s: NULL pointer", who);
  VIRNET_REQUIRE(nsrc >= 1 && nsrc <= kMax, "%s: %d source tensors (1 .. %d expected)", who, nsrc, kMax);
  VIRNET_REQUIRE(aligned(log, 8), "%s: the log must be 8-byte aligned", who);
  PushArgs a{};
  int total = 0;
  for (int s = 0; s < nsrc; ++s) {
    VIRNET_REQUIRE(src[s] != nullptr, "%s: source %d is NULL", who, s);
    VIRNET_REQUIRE(aligned(src[s], 4), "%s: source %d is misaligned", who, s);
    VIRNET_REQUIRE(count[s] >= 1 && count[s] <= kMax, "%s: source %d holds %d values (1 .. %d expected)", who, s, count[s], kMax);
    a.src[s] = static_cast<const float*>(src[s]);
    a.first[s] = total;
    total += count[s];
    VIRNET_REQUIRE(total <= kMax, "%s: more than %d values", who, kMax);
  }
  VIRNET_REQUIRE(total == k, "%s: the sources hold %d values, the log %d", who, total, k);
  for (int s = nsrc; s <= kMax; ++s) a.first[s] = k;
  for (int s = nsrc; s < kMax; ++s) a.src[s] = a.src[0];
  const unsigned long long log_bytes = (unsigned long long)k * 8ull + (unsigned long long)capacity * k * 4ull;
  const uintptr_t lo = (uintptr_t)log, hi = lo + log_bytes;
  for (int s = 0; s < nsrc; ++s) {
    const uintptr_t p = (uintptr_t)src[s];
    VIRNET_REQUIRE(p + 4ull * count[s] <= lo || hi <= p, "%s: source %d lies inside the log", who, s);
  }
  a.nsrc = nsrc; a.k = k; a.num_iter = num_iter;
  a.sums = static_cast<double*>(log);
  a.row = reinterpret_cast<float*>(static_cast<unsigned char*>(log) + (size_t)k * 8) + (size_t)slot * k;
  hipLaunchKernelGGL(trainlog_push_kernel, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return virnet::check_launch("trainlog push launch");
}

extern "C" int virnet_trainlog_reset(void* log, int k, void* stream) {
  const char* const who = "virnet_trainlog_reset";
  VIRNET_REQUIRE(k >= 1 && k <= kMax, "%s: %d values (1 .. %d expected)", who, k, kMax);
  VIRNET_REQUIRE(log && aligned(log, 8), "%s: the log must be a non-NULL 8-byte aligned pointer", who);
  hipLaunchKernelGGL(trainlog_reset_kernel, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream), static_cast<double*>(log), k);
  return virnet::check_launch("trainlog reset launch");
}
