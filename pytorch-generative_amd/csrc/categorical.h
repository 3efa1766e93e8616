// categorical.h — the two device rules the K-way softmax kernels share (categorical.hip, linear_categorical.hip).
#pragma once
#include <math.h>

#include "common.h"

// the class of an image value at the levels j / (K - 1)
__device__ __forceinline__ int cat_class(float x, int K) {
  // fmaxf / fminf drop a NaN: the index is in range whatever the image holds
  return (int)fminf(fmaxf(rintf(x * (float)(K - 1)), 0.f), (float)(K - 1));
}

// (m, s) stands for m + log s; (-inf, 0) is the empty sum. All-(-inf) inputs keep it empty (no exp(-inf + inf)).
__device__ __forceinline__ void cat_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  const float ref = mn > -INFINITY ? mn : 0.f;
  s = s * __expf(m - ref) + s2 * __expf(m2 - ref);
  m = mn;
}
