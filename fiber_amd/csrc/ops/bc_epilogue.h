// The behaviour-characterisation epilogue shared by the rollout kernels that
// report a BC: es_rollout_mlp_bc and es_eval_bc (ns_kernels.hip) and
// ga_rollout_mlp_bc (me_kernels.hip).  Include after the shared device code
// of es_kernels.hip, which defines RolloutLds, ENVS and OBS.
#pragma once

// BC epilogue of both kernels.  Call after rollout_steps has returned: its
// closing barrier is behind every thread, step t wrote L.S[(t & 1) ^ 1],
// so s_H[env][d] is L.S[horizon & 1][env][d] (s_0 in L.S[0] for the
// degenerate horizon 0 too), and nothing writes L.S afterwards.  Thread
// (env = tid & 63, d = tid >> 6) reads its own component; wave d sums the
// 64 envs of dim d with the fixed shuffle tree of psum / psq, so the order
// of the adds is the same every run (no atomics), and lane 0 divides by 64
// (exact).  bc4 -> this block's 4 floats, final_states -> its [ENVS][OBS]
// floats or null.
__device__ __forceinline__ void bc_reduce_store(
    const RolloutLds& L, int tid, int horizon, float* __restrict__ bc4,
    float* __restrict__ final_states) {
  const int env = tid & 63;
  const int dd = tid >> 6;  // 0..3
  const float s = L.S[horizon & 1][env][dd];
  if (final_states != nullptr) final_states[env * OBS + dd] = s;
  float acc = s;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (env == 0) bc4[dd] = acc / (float)ENVS;
}
