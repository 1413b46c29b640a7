// float32 -> uint8 of the evaluation tables, shared by metrics.hip (virnet_quantize_u8, the metric kernels) and ensemble.hip (the
// self-ensemble's uint8 output): bit for bit eval.img_as_ubyte after the tables' clip.
#pragma once
#include <hip/hip_runtime.h>

namespace virnet {

// clamp to [0,1] in fp32 (NaN and -0 -> +0)
__device__ __forceinline__ float clip01(float x) { return x > 0.f ? (x < 1.f ? x : 1.f) : 0.f; }

// (double)x * 255.0 is exact (24 x 8 bits); rint rounds half to even like np.rint
__device__ __forceinline__ unsigned quant_u8(float x) { return (unsigned)(int)rint((double)clip01(x) * 255.0); }

}  // namespace virnet
