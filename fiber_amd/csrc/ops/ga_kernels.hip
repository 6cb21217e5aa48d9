// Deep GA kernels (Such et al., "Deep Neuroevolution: Genetic Algorithms Are
// a Competitive Alternative for Training Deep Neural Networks for
// Reinforcement Learning"): truncation selection over a population in which
// every member is a Gaussian mutation of one of T parents, stored as its
// chain of mutation seeds.
//
//   ga_parents      who mutates whom: parent_idx[pop], slot[pop]
//   ga_rollout_mlp  es_rollout_mlp with a parent row and a draw per member
//   ga_truncate     order[T]: the indices of the T best, exact tie order
//   ga_survivors    new_parents[T][NPARAMS]: the weights the survivors were
//                   evaluated with
//   ga_decode       weights from seed chains: theta0 plus every mutation of
//                   a lineage row, in generation order
//
// Noise convention.  The mutation of child slot i in generation g is
// fam_normal4(seed, g, i, jb, FAM_TAG_NOISE, 0u, z): the draw es_rollout_mlp
// uses for pair i at iteration g.  Episodes of generation g start from
// rollout_init_lds(..., seed, g).
//
// The multiply-add.  A mutated weight is ga_mutate(parent, sigma, z) =
// fmaf(sigma, z, parent), spelled out, in ga_rollout_mlp, ga_survivors and
// ga_decode alike.  es_rollout_mlp writes theta[j] + sgn * z[u] and leaves
// the fusing to the compiler, which contracts it to one v_fmac_f32 there
// (profiles/snes.md, profiles/ga.md); an explicit fma of the same three
// operands is that instruction's result, so an even member of es_rollout_mlp
// and a mutated member here carry the same bits.  The plain expression would
// do the same today, but whether it is contracted is decided per use: in
// ga_decode the add sits in a loop with a branch around it, in ga_survivors
// next to a copy, and one of them compiled as multiply then add would be
// off by a rounding from the other two with nothing in the source to show
// it.  With fmaf the three cannot come apart, which is what lets
// ga_decode(lineage) equal the materialised parents bit for bit
// (tests/gpu/test_ga_gpu.py).
//
// The shared device code of es_kernels.hip is included below without its
// kernels, as es_pairs_kernels.hip, ns_kernels.hip and snes_kernels.hip do,
// and for the same reason: this is a translation unit of its own so that
// its instantiation of rollout_steps cannot move the register allocation of
// es_rollout_mlp and es_eval_matrix, which sit 3 and 4 VGPRs under their
// budget (profiles/es_population.md, profiles/ga.md).

#define ES_KERNELS_SHARED_ONLY
#include "es_kernels.hip"

// Philox tag of the parent draw; 0x45530001..3 are noise, env and conv obs.
#define FAM_TAG_GA_PARENT 0x45530004u

// ga_mutate and ga_rank_key, shared with me_kernels.hip
#include "ga_shared.h"

// Member m < n_elite is survivor m of the last generation, unmutated
// (slot -1).  Every other member mutates a uniformly drawn survivor with the
// draw of its own slot: parent = floor(u * T_cur / 2^32), u one Philox word.
// Integer only (fiber_amd/es/ga_oracle.py: parents_exact).
extern "C" __global__ void ga_parents(uint32_t seed, uint32_t gen, int pop,
                                      int n_elite, uint32_t T_cur,
                                      int* __restrict__ parent_idx,
                                      int* __restrict__ slot) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= pop) return;
  if (m < n_elite) {
    parent_idx[m] = m;
    slot[m] = -1;
    return;
  }
  const fam_uint4 u =
      philox4x32_10(seed, gen, (uint32_t)m, 0u, FAM_TAG_GA_PARENT, 0u);
  parent_idx[m] = (int)fam_mulhi(u.x, T_cur);
  slot[m] = m;
}

// es_rollout_mlp with a parent row and a draw per member.  LDS init, step
// loop and the fitness / obs-stat epilogue are that kernel's, line for
// line; only the policy fill differs.  parent_idx[m] must lie in [0, T) and
// sigma must be finite (not checked here).  The branch is uniform over the
// block.
extern "C" __global__ void __launch_bounds__(256, ROLLOUT_WAVES)
ga_rollout_mlp(const float* __restrict__ parents,   // [T][NPARAMS]
               const int* __restrict__ parent_idx,  // [pop]
               const int* __restrict__ slot,        // [pop]
               float sigma, uint32_t seed, uint32_t gen, int horizon,
               const float* __restrict__ obs_mu,
               const float* __restrict__ obs_nu,
               const float* __restrict__ env_A,    // [OBS][OBS]
               const float* __restrict__ env_B,    // [OBS]
               float* __restrict__ fitness,        // [pop]
               float* __restrict__ obs_stat_part,  // [pop][2*OBS]
               float* __restrict__ obs_stat_out)   // [2*OBS+1]
{
  __shared__ RolloutLds L;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const float* __restrict__ theta =
      parents + (size_t)parent_idx[blockIdx.x] * NPARAMS;
  const int sl = slot[blockIdx.x];

  // ---- fill the member's policy into LDS ------------------------------
  if (sl < 0) {
    // an unmutated elite: es_eval_matrix's loop, no Philox, no add
    for (int j = tid; j < NPARAMS; j += blockDim.x)
      store_param(&L.pol, j, theta[j]);
  } else {
    for (int jb = tid; jb * 4 < NPARAMS; jb += blockDim.x) {
      float z[4];
      fam_normal4(seed, gen, (uint32_t)sl, (uint32_t)jb, FAM_TAG_NOISE, 0u,
                  z);
      const int j0 = jb * 4;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u;
        if (j < NPARAMS)
          store_param(&L.pol, j, ga_mutate(theta[j], sigma, z[u]));
      }
    }
  }
  rollout_init_lds<true>(L, tid, seed, gen);
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
// Truncation selection: order[r] = the member of descending rank r < T,
//   rank(i) = #{j : f[j] > f[i] or (f[j] == f[i] and j < i)},
// a NaN below every number, NaNs among themselves by index, -0 == +0.
//
// The fitness becomes an unsigned key whose integer order is that order
// (rank_pack_keys' sign flip, with both zeros on one key and every NaN on
// key 0, under -inf's 0x007fffff), so the count is integer compares only.
// Comparison counting, as centered_rank does: every block stages the keys
// tile by tile in LDS and each thread counts the members that beat its own.
// The ranks are a permutation of 0..n-1, so each order[r] is written once.
// O(n^2 / threads) with n <= 65536: about 16 million LDS broadcast reads
// per wave at the largest n, next to a rollout launch of tens of
// milliseconds.
// ---------------------------------------------------------------------------
#define GA_TRUNC_TILE 2048

extern "C" __global__ void __launch_bounds__(256)
ga_truncate(const float* __restrict__ f, int n, int T,
            int* __restrict__ order) {
  __shared__ unsigned keys[GA_TRUNC_TILE];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  // threads past n keep walking: they take part in the barriers
  const unsigned ki = i < n ? ga_rank_key(f[i]) : 0u;
  int rank = 0;
  for (int base = 0; base < n; base += GA_TRUNC_TILE) {
    const int len = min(GA_TRUNC_TILE, n - base);
    __syncthreads();  // the previous tile has been read
    for (int k = threadIdx.x; k < len; k += blockDim.x)
      keys[k] = ga_rank_key(f[base + k]);
    __syncthreads();
    // members before i win a tie, members after it lose it
    const int before = min(max(i - base, 0), len);
    for (int k = 0; k < before; ++k) rank += keys[k] >= ki;
    for (int k = before; k < len; ++k) rank += keys[k] > ki;
  }
  // i itself fell into the second loop, where its own key does not count
  if (i < n && rank < T) order[rank] = i;
}

// new_parents[t] = the weights member order[t] was evaluated with: its
// parent row as it is for slot < 0, otherwise ga_rollout_mlp's multiply-add
// from the same draw.  grid.x tiles the parameter blocks, grid.y is t.  Out
// of place: new_parents must not alias parents.
extern "C" __global__ void ga_survivors(
    const float* __restrict__ parents,   // [T_cur][NPARAMS]
    const int* __restrict__ parent_idx,  // [pop]
    const int* __restrict__ slot,        // [pop]
    const int* __restrict__ order,       // [T]
    float sigma, uint32_t seed, uint32_t gen,
    float* __restrict__ new_parents)     // [T][NPARAMS]
{
  const int jb = blockIdx.x * blockDim.x + threadIdx.x;
  if (jb * 4 >= NPARAMS) return;
  const int m = order[blockIdx.y];
  const float* __restrict__ theta = parents + (size_t)parent_idx[m] * NPARAMS;
  const int sl = slot[m];
  float* __restrict__ row = new_parents + (size_t)blockIdx.y * NPARAMS;
  float z[4] = {0.f, 0.f, 0.f, 0.f};
  if (sl >= 0)
    fam_normal4(seed, gen, (uint32_t)sl, (uint32_t)jb, FAM_TAG_NOISE, 0u, z);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int j = jb * 4 + u;
    if (j < NPARAMS)
      row[j] = sl >= 0 ? ga_mutate(theta[j], sigma, z[u]) : theta[j];
  }
}

// thetas[n] = theta0 with the mutations of lineage row n applied in
// generation order: column c holds the slot drawn in generation c, or -1
// for a generation the genome passed through unmutated.  The fold is the
// one ga_survivors performs generation by generation, with the same
// multiply-add, so the result carries the bits of the materialised parents.
// grid.x tiles the parameter blocks, grid.y is n.
extern "C" __global__ void ga_decode(
    const float* __restrict__ theta0,  // [NPARAMS]
    const int* __restrict__ lineage,   // [N][G]
    int G, float sigma, uint32_t seed,
    float* __restrict__ thetas)        // [N][NPARAMS]
{
  const int jb = blockIdx.x * blockDim.x + threadIdx.x;
  if (jb * 4 >= NPARAMS) return;
  const int* __restrict__ chain = lineage + (size_t)blockIdx.y * G;
  float acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int j = jb * 4 + u;
    acc[u] = j < NPARAMS ? theta0[j] : 0.f;
  }
  for (int c = 0; c < G; ++c) {
    const int sl = chain[c];
    if (sl < 0) continue;
    float z[4];
    fam_normal4(seed, (uint32_t)c, (uint32_t)sl, (uint32_t)jb, FAM_TAG_NOISE,
                0u, z);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = ga_mutate(acc[u], sigma, z[u]);
  }
  float* __restrict__ row = thetas + (size_t)blockIdx.y * NPARAMS;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int j = jb * 4 + u;
    if (j < NPARAMS) row[j] = acc[u];
  }
}
