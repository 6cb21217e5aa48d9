// Separable-NES kernels: what learning a step size per parameter needs and
// the scalar-sigma kernels cannot do.
//
//   es_rollout_mlp_sigma  es_rollout_mlp with sigma[NPARAMS] instead of a
//                         scalar: parameter j is theta[j] +- sigma[j] * z
//   es_grad_sigma         es_grad with two rows from ONE regeneration of the
//                         draws: g_mu[j]  = sum_k wdiff[k] * z_k[j]
//                                g_sig[j] = sum_k wsum[k] * (z_k[j]^2 - 1)
//
// es_rollout_mlp_sigma writes, for a uniform sigma vector, the bits of
// es_rollout_mlp: the perturbation is the same single multiply-add, and
// LDS init, step loop and epilogue are the functions that kernel inlines
// (tests/gpu/test_snes_gpu.py).  The g_mu row carries the bits of
// es_grad(wdiff): the same accumulate over the same chunk split, reduced
// by the same es_grad_reduce.
//
// The shared device code of es_kernels.hip is included below without its
// kernels, as es_pairs_kernels.hip and ns_kernels.hip do, and for the same
// reason: this is a translation unit of its own so that its instantiation
// of rollout_steps cannot move the register allocation of es_rollout_mlp
// and es_eval_matrix, which sit 3 and 4 VGPRs under their budget
// (profiles/es_population.md, profiles/snes.md).

#define ES_KERNELS_SHARED_ONLY
#include "es_kernels.hip"

// es_rollout_mlp with a step size per parameter.  Arguments, LDS init,
// step loop and the fitness / obs-stat epilogue are that kernel's, line for
// line; only the policy fill differs.  sigma[j] must be finite and >= 0
// (not checked here).  The 18 KB vector is read once per block, before the
// step loop, and stays in L2 across the grid.
extern "C" __global__ void __launch_bounds__(256, ROLLOUT_WAVES)
es_rollout_mlp_sigma(const float* __restrict__ theta,
                     const float* __restrict__ sigma,  // [NPARAMS]
                     uint32_t seed, uint32_t iter, int horizon,
                     int member_offset, const float* __restrict__ obs_mu,
                     const float* __restrict__ obs_nu,
                     const float* __restrict__ env_A,    // [OBS][OBS]
                     const float* __restrict__ env_B,    // [OBS]
                     float* __restrict__ fitness,        // [pop_shard]
                     float* __restrict__ obs_stat_part,  // [pop_shard][2*OBS]
                     float* __restrict__ obs_stat_out)   // [2*OBS+1]
{
  __shared__ RolloutLds L;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int member = member_offset + blockIdx.x;
  const uint32_t pair = (uint32_t)(member >> 1);
  const bool odd = member & 1;

  // ---- fill perturbed policy into LDS ---------------------------------
  // theta[j] + sgn * z[u] is es_rollout_mlp's expression with sgn taken
  // per parameter: the compiler contracts both to one fma, and negating
  // sigma[j] is exact.
  for (int jb = tid; jb * 4 < NPARAMS; jb += blockDim.x) {
    float z[4];
    fam_normal4(seed, iter, pair, (uint32_t)jb, FAM_TAG_NOISE, 0u, z);
    const int j0 = jb * 4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u;
      if (j < NPARAMS) {
        const float sgn = odd ? -sigma[j] : sigma[j];
        store_param(&L.pol, j, theta[j] + sgn * z[u]);
      }
    }
  }
  rollout_init_lds<true>(L, tid, seed, iter);
  __syncthreads();

  const int env = tid & 63;
  const int dd = tid >> 6;  // 0..3
  float psum = 0.f, psq = 0.f;
  const float raccp = rollout_steps<true>(L, tid, horizon, obs_mu, obs_nu,
                                          env_A, env_B, psum, psq);

  // ---- epilogue: fitness + obs-stat reductions (es_rollout_mlp's) ------
  L.lpart[dd][env][0] = raccp;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    psum += __shfl_down(psum, off, 64);
    psq += __shfl_down(psq, off, 64);
  }
  if (lane == 0) {
    L.ostat[dd] = psum;
    L.ostat[OBS + dd] = psq;
  }
  __syncthreads();
  if (wave == 0) {
    const float r = reward_reduce_wave0(L, lane, nullptr);
    if (lane == 0) fitness[blockIdx.x] = r / (float)ENVS;
  }
  // per-member partials; obs_stat_reduce sums them in a fixed order
  if (tid < 2 * OBS)
    obs_stat_part[(size_t)blockIdx.x * (2 * OBS) + tid] = L.ostat[tid];
  // every block adds the same value, so the order cannot change the sum
  if (tid == 0)
    atomicAdd(&obs_stat_out[2 * OBS], (float)(ENVS * horizon));
}

// ---------------------------------------------------------------------------
// Two-row gradient: grid, chunk split and partial layout are es_grad's,
// with 2*nparams floats per chunk row, [g_mu | g_sig].  grid.x tiles the
// parameter blocks, grid.y the local pair range.  Each draw is regenerated
// once and feeds both rows.
//
// The g_mu accumulate is es_grad's statement, so it contracts to the same
// fma.  es_grad skips a pair whose weight is 0; here a pair is skipped only
// when both weights are 0, and where one of them is, fma(0, z, acc) leaves
// acc as it is: z is finite and acc is never -0 (it starts at +0, and a
// round-to-nearest sum is -0 only if both addends are).  The g_sig terms
// are spelled out, one rounding each: q = fma(z, z, -1), acc = fma(w, q,
// acc).
// ---------------------------------------------------------------------------
extern "C" __global__ void es_grad_sigma(const float* __restrict__ wdiff,
                                         const float* __restrict__ wsum,
                                         int pair_begin, int pair_end,
                                         int pairs_per_chunk, uint32_t seed,
                                         uint32_t iter, int nparams,
                                         float* __restrict__ out) {
  const int jb = blockIdx.x * blockDim.x + threadIdx.x;
  if (jb * 4 >= nparams) return;
  const int chunk_begin = pair_begin + blockIdx.y * pairs_per_chunk;
  const int chunk_end = min(chunk_begin + pairs_per_chunk, pair_end);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  float acs[4] = {0.f, 0.f, 0.f, 0.f};
  for (int pair = chunk_begin; pair < chunk_end; ++pair) {
    const float w = wdiff[pair];
    const float ws = wsum[pair];
    if (w == 0.f && ws == 0.f) continue;
    float z[4];
    fam_normal4(seed, iter, (uint32_t)pair, (uint32_t)jb, FAM_TAG_NOISE, 0u,
                z);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] += w * z[u];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      acs[u] = fmaf(ws, fmaf(z[u], z[u], -1.0f), acs[u]);
  }
  // Each (chunk, row, j) is written by exactly one thread.  With one chunk
  // `out` is the [2][nparams] result itself; otherwise it is the
  // [chunks][2*nparams] partial buffer that es_grad_reduce sums in chunk
  // order over 2*nparams columns (no float atomics).
  float* __restrict__ row = out + (size_t)blockIdx.y * 2 * nparams;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int j = jb * 4 + u;
    if (j < nparams) {
      row[j] = acc[u];
      row[(size_t)nparams + j] = acs[u];
    }
  }
}
