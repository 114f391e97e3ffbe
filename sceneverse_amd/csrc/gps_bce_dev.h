// gps_bce_dev.h -- the two device functions of BCEWithLogits shared by the answer loss (gps_qa.hip) and the BCE branch of
// TextObjWithinBatch (gps_contrastive.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace gps_bce {

// max(x, 0) - x y + log1p(exp(-|x|)): no overflow for any x
__device__ __forceinline__ float bce_term(float x, float y) { return fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoidf(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

}  // namespace gps_bce
