// Per-pair batched ES kernels: P independent (policy, environment) pairs,
// a POET population, advanced by one launch each instead of one launch
// per pair.  Every pair brings its own theta, obs normaliser, environment
// and noise seed; sigma, iter and horizon are shared.
//
// Each kernel here is the per-pair form of one in es_kernels.hip and must
// give, for pair p, the bits that kernel gives when launched for pair p
// alone (tests/gpu/test_es_population.py):
//
//   es_rollout_mlp_pairs   es_rollout_mlp at member_offset 0, pop_shard pop
//   obs_stat_reduce_pairs  obs_stat_reduce over the pair's pop partials
//   centered_rank_pairs    centered_rank (the O(n^2) kernel) on one row
//   es_grad_pairs          es_grad + es_grad_reduce, same chunk split
//
// The rollout kernel inlines the very functions that es_rollout_mlp and
// es_eval_matrix inline (rollout_init_lds, rollout_steps,
// reward_reduce_wave0), so the step arithmetic cannot drift: the shared
// device code of es_kernels.hip is included below, without its kernels.
// This file is a translation unit of its own so that its instantiation of
// rollout_steps cannot move the register allocation of those two, which
// sit 3 and 4 VGPRs under their budget (profiles/es_population.md).

#define ES_KERNELS_SHARED_ONLY
#include "es_kernels.hip"

// One workgroup per (pair, member), flattened into blockIdx.x as
// es_eval_matrix does (p = block / pop, member = block % pop): P * pop
// outgrows gridDim.y.  Block (p, member) is block `member` of
// es_rollout_mlp launched for pair p with member_offset 0.
extern "C" __global__ void __launch_bounds__(256, ROLLOUT_WAVES)
es_rollout_mlp_pairs(const float* __restrict__ thetas,  // [P][NPARAMS]
                     float sigma,
                     const uint32_t* __restrict__ seeds,  // [P]
                     uint32_t iter, int horizon, int pop,
                     const float* __restrict__ obs_mu,  // [P][OBS]
                     const float* __restrict__ obs_nu,  // [P][OBS]
                     const float* __restrict__ env_A,   // [P][OBS][OBS]
                     const float* __restrict__ env_B,   // [P][OBS]
                     float* __restrict__ fitness,        // [P][pop]
                     float* __restrict__ obs_stat_part,  // [P][pop][2*OBS]
                     float* __restrict__ obs_stat_out)   // [P][2*OBS+1]
{
  __shared__ RolloutLds L;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const size_t p = blockIdx.x / (unsigned)pop;  // P * pop < 2^31
  const int member = (int)(blockIdx.x % (unsigned)pop);
  const uint32_t seed = seeds[p];
  const float* __restrict__ theta = thetas + p * NPARAMS;
  const uint32_t pair = (uint32_t)(member >> 1);
  const float sgn = (member & 1) ? -sigma : sigma;

  // ---- fill perturbed policy into LDS ---------------------------------
  for (int jb = tid; jb * 4 < NPARAMS; jb += blockDim.x) {
    float z[4];
    fam_normal4(seed, iter, pair, (uint32_t)jb, FAM_TAG_NOISE, 0u, z);
    const int j0 = jb * 4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u;
      if (j < NPARAMS) store_param(&L.pol, j, theta[j] + sgn * z[u]);
    }
  }
  rollout_init_lds<true>(L, tid, seed, iter);
  __syncthreads();

  const int env = tid & 63;
  const int dd = tid >> 6;  // 0..3
  float psum = 0.f, psq = 0.f;
  const float raccp = rollout_steps<true>(
      L, tid, horizon, obs_mu + p * OBS, obs_nu + p * OBS,
      env_A + p * (OBS * OBS), env_B + p * OBS, psum, psq);

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
  // per-member partials; obs_stat_reduce_pairs sums them in a fixed order
  if (tid < 2 * OBS)
    obs_stat_part[(size_t)blockIdx.x * (2 * OBS) + tid] = L.ostat[tid];
  // every block of a pair adds the same value to the pair's count, so the
  // order cannot change the sum
  if (tid == 0)
    atomicAdd(&obs_stat_out[p * (2 * OBS + 1) + 2 * OBS],
              (float)(ENVS * horizon));
}

// obs_stat_out[p][c] = sum over the pair's members of part[p][m][c]: block
// (c, p) runs obs_stat_reduce's strided accumulation and LDS tree over
// pair p's partials, so the order of the adds is the one that kernel uses
// for nmembers = pop.
extern "C" __global__ void __launch_bounds__(256)
obs_stat_reduce_pairs(const float* __restrict__ part,  // [P][pop][2*OBS]
                      int pop,
                      float* __restrict__ obs_stat_out)  // [P][2*OBS+1]
{
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const int col = blockIdx.x;  // grid is exactly (2*OBS, P)
  const size_t p = blockIdx.y;
  const float* __restrict__ rows = part + p * (size_t)pop * (2 * OBS);
  float acc = 0.f;
  for (int m = tid; m < pop; m += 256)
    acc += rows[(size_t)m * (2 * OBS) + col];
  red[tid] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) obs_stat_out[p * (2 * OBS + 1) + col] = red[0];
}

// out[p][i] = rank of f[p][i] within row p, centered: centered_rank's
// O(n^2) comparison with its index-order tie-break, one grid row per pair.
extern "C" __global__ void centered_rank_pairs(
    const float* __restrict__ f,  // [P][n]
    int n, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* __restrict__ row = f + (size_t)blockIdx.y * n;
  const float fi = row[i];
  int rank = 0;
  for (int j = 0; j < n; ++j) {
    const float fj = row[j];
    rank += (fj < fi) || (fj == fi && j < i);
  }
  out[(size_t)blockIdx.y * n + i] = (float)rank / (float)(n - 1) - 0.5f;
}

// es_grad for every pair: grid.x tiles the parameter blocks, grid.y the
// chunks of the Philox pair range [0, npairs), grid.z the P pairs.  `out`
// is grad[P][nparams] when there is one chunk, else the partial buffer
// [P][chunks][nparams] that es_grad_reduce_pairs sums in chunk order.
extern "C" __global__ void es_grad_pairs(
    const float* __restrict__ wpair,     // [P][npairs]
    int npairs, int pairs_per_chunk,
    const uint32_t* __restrict__ seeds,  // [P]
    uint32_t iter, int nparams, float* __restrict__ out) {
  const int jb = blockIdx.x * blockDim.x + threadIdx.x;
  if (jb * 4 >= nparams) return;
  const size_t p = blockIdx.z;
  const uint32_t seed = seeds[p];
  const float* __restrict__ w_row = wpair + p * (size_t)npairs;
  const int chunk_begin = blockIdx.y * pairs_per_chunk;
  const int chunk_end = min(chunk_begin + pairs_per_chunk, npairs);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int pair = chunk_begin; pair < chunk_end; ++pair) {
    const float w = w_row[pair];
    if (w == 0.f) continue;
    float z[4];
    fam_normal4(seed, iter, (uint32_t)pair, (uint32_t)jb, FAM_TAG_NOISE, 0u,
                z);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] += w * z[u];
  }
  // each (pair, chunk, j) is written by exactly one thread
  float* __restrict__ row =
      out + (p * gridDim.y + blockIdx.y) * (size_t)nparams;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int j = jb * 4 + u;
    if (j < nparams) row[j] = acc[u];
  }
}

extern "C" __global__ void es_grad_reduce_pairs(
    const float* __restrict__ part,  // [P][chunks][nparams]
    int chunks, int nparams,
    float* __restrict__ grad)  // [P][nparams]
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nparams) return;
  const size_t p = blockIdx.y;
  const float* __restrict__ rows = part + p * (size_t)chunks * nparams;
  float acc = 0.f;
  for (int c = 0; c < chunks; ++c) acc += rows[(size_t)c * nparams + j];
  grad[p * (size_t)nparams + j] = acc;
}
