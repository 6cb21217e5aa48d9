// Device functions that the Deep GA kernels (ga_kernels.hip) and the
// MAP-Elites kernels (me_kernels.hip) must agree on bit for bit: the
// mutation multiply-add and the fitness order key.  One text, included by
// both translation units, so the two cannot come apart.
#pragma once

__device__ __forceinline__ float ga_mutate(float parent, float sigma,
                                           float z) {
  return fmaf(sigma, z, parent);
}

__device__ __forceinline__ unsigned ga_rank_key(float f) {
  if (f != f) return 0u;
  unsigned u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
