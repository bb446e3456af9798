// The row softmax every kernel of the library evaluates the same way: l = row_lse(z, C), p_c = row_softmax_at(z, l, c).  One definition,
// so that a kernel that forms probabilities on the fly (lovasz.hip) gets the bits mopa_softmax_fwd (losses.hip) stores.
// Included after common.h.
#pragma once

__device__ __forceinline__ float row_lse(const float* __restrict__ z, int C) {
  float mx = z[0];
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, z[c]);
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += expf(z[c] - mx);
  return mx + logf(s);
}

__device__ __forceinline__ float row_softmax_at(float zc, float lse) { return expf(zc - lse); }
