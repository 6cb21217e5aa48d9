// Novelty-search ES kernels: the two MLP rollout kernels extended by a
// behaviour characterisation (BC), and k-nearest-neighbour novelty of BCs
// against an archive.
//
// The BC of a member (or of a policy x environment cell) is the mean over
// its 64 episodes of the final state s_H, 4 floats.  It is read after the
// shared step loop has returned, so the loop itself is not touched:
//
//   es_rollout_mlp_bc  es_rollout_mlp  + bc[pop_shard][4]
//   es_eval_bc         es_eval_matrix  + bc[K][M][4]
//
// and both may also store the 64 final states themselves.  Everything the
// two siblings write, these write with the same bits: they inline the very
// functions those inline (rollout_init_lds, rollout_steps,
// reward_reduce_wave0) and repeat their epilogues
// (tests/gpu/test_novelty_es_gpu.py).
//
// The shared device code of es_kernels.hip is included below without its
// kernels, as es_pairs_kernels.hip does, and for the same reason: this is
// a translation unit of its own so that its instantiations of
// rollout_steps cannot move the register allocation of es_rollout_mlp and
// es_eval_matrix, which sit 3 and 4 VGPRs under their budget
// (profiles/es_population.md, profiles/novelty_es.md).

#define ES_KERNELS_SHARED_ONLY
#include "es_kernels.hip"

// bc_reduce_store, the BC epilogue of both kernels, shared with
// me_kernels.hip
#include "bc_epilogue.h"

// es_rollout_mlp with a BC per member.  Arguments, policy fill, LDS init,
// step loop and the fitness / obs-stat epilogue are that kernel's, line
// for line; only the last call is new.
extern "C" __global__ void __launch_bounds__(256, ROLLOUT_WAVES)
es_rollout_mlp_bc(const float* __restrict__ theta, float sigma,
                  uint32_t seed, uint32_t iter, int horizon,
                  int member_offset, const float* __restrict__ obs_mu,
                  const float* __restrict__ obs_nu,
                  const float* __restrict__ env_A,    // [OBS][OBS]
                  const float* __restrict__ env_B,    // [OBS]
                  float* __restrict__ fitness,        // [pop_shard]
                  float* __restrict__ obs_stat_part,  // [pop_shard][2*OBS]
                  float* __restrict__ obs_stat_out,   // [2*OBS+1]
                  float* __restrict__ bc,             // [pop_shard][OBS]
                  float* __restrict__ final_states)   // [pop_shard][ENVS][OBS]
                                                      // or null
{
  __shared__ RolloutLds L;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int member = member_offset + blockIdx.x;
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
  if (tid < 2 * OBS)
    obs_stat_part[(size_t)blockIdx.x * (2 * OBS) + tid] = L.ostat[tid];
  if (tid == 0)
    atomicAdd(&obs_stat_out[2 * OBS], (float)(ENVS * horizon));

  // ---- behaviour characterisation --------------------------------------
  bc_reduce_store(L, tid, horizon, bc + (size_t)blockIdx.x * OBS,
                  final_states != nullptr
                      ? final_states + (size_t)blockIdx.x * (ENVS * OBS)
                      : nullptr);
}

// es_eval_matrix with a BC per cell: K explicit policies x M environments,
// the cell index flattened into blockIdx.x (k = cell / M, m = cell % M).
extern "C" __global__ void __launch_bounds__(256, ROLLOUT_WAVES)
es_eval_bc(const float* __restrict__ thetas,  // [K][NPARAMS]
           const float* __restrict__ obs_mu,  // [K][OBS]
           const float* __restrict__ obs_nu,  // [K][OBS]
           const float* __restrict__ env_A,   // [M][OBS][OBS]
           const float* __restrict__ env_B,   // [M][OBS]
           uint32_t seed, uint32_t iter, int horizon, int M,
           float* __restrict__ scores,        // [K][M]
           float* __restrict__ episodes,      // [K][M][ENVS] or null
           float* __restrict__ bc,            // [K][M][OBS]
           float* __restrict__ final_states)  // [K][M][ENVS][OBS] or null
{
  __shared__ RolloutLds L;
  const int tid = threadIdx.x;
  const size_t cell = blockIdx.x;
  const size_t k = cell / (size_t)M;
  const size_t m = cell % (size_t)M;

  const float* __restrict__ theta = thetas + k * NPARAMS;
  for (int j = tid; j < NPARAMS; j += blockDim.x)
    store_param(&L.pol, j, theta[j]);
  rollout_init_lds<false>(L, tid, seed, iter);
  __syncthreads();

  float psum = 0.f, psq = 0.f;  // unused: STATS=false compiles them out
  const float raccp = rollout_steps<false>(
      L, tid, horizon, obs_mu + k * OBS, obs_nu + k * OBS,
      env_A + m * (OBS * OBS), env_B + m * OBS, psum, psq);

  L.lpart[tid >> 6][tid & 63][0] = raccp;
  __syncthreads();
  if (tid < 64) {
    const float r = reward_reduce_wave0(
        L, tid, episodes != nullptr ? episodes + cell * ENVS : nullptr);
    if (tid == 0) scores[cell] = r / (float)ENVS;
  }

  bc_reduce_store(L, tid, horizon, bc + cell * OBS,
                  final_states != nullptr
                      ? final_states + cell * (ENVS * OBS)
                      : nullptr);
}

// ---------------------------------------------------------------------------
// k-nearest-neighbour novelty of BCs against an archive.
//
// novelty[q] = mean of the k smallest Euclidean distances from bc[q] to
// the R archive rows; knn_d2[q][0..k) = the k smallest squared distances,
// ascending (optional).  Duplicate archive rows are separate neighbours.
//
// One thread per query, 256 per block.  The archive streams through LDS in
// tiles of BC_KNN_TILE rows held as float4: in the scan every lane reads
// the same row, a broadcast, so there are no bank conflicts.  Each thread
// keeps its BC_KNN_MAX best squared distances sorted in registers; a
// candidate under the current worst is placed by a fully unrolled
// compare-and-shift (best[] is only ever indexed by constants, so it never
// goes to scratch).  k <= BC_KNN_MAX only selects how many are reported.
//
// The squared distance is spelled out, one rounding per line, so that no
// schedule can contract it differently:
//   d_i = q_i - a_i;  acc = d_0 * d_0;  acc = fma(d_i, d_i, acc), i = 1..3
// and sqrtf is taken once per reported entry.  Inputs must be finite: with
// a NaN or an infinity in a BC the ordering of the list, and with it the
// novelty, is unspecified.
// ---------------------------------------------------------------------------
#define BC_KNN_MAX 16
#define BC_KNN_TILE 1024  // rows per LDS tile: 16 KB

extern "C" __global__ void __launch_bounds__(256)
bc_knn_novelty(const float* __restrict__ bc,       // [N][OBS]
               int N,
               const float* __restrict__ archive,  // [R][OBS]
               int R, int k,
               float* __restrict__ novelty,        // [N]
               float* __restrict__ knn_d2)         // [N][k] or null
{
  static_assert(OBS == 4, "BC rows are read as float4");
  __shared__ float4 tile[BC_KNN_TILE];
  const int tid = threadIdx.x;
  const int q = blockIdx.x * 256 + tid;
  const bool live = q < N;  // the others only help to stage the tiles
  float4 qv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) qv = reinterpret_cast<const float4*>(bc)[q];

  float best[BC_KNN_MAX];
#pragma unroll
  for (int j = 0; j < BC_KNN_MAX; ++j) best[j] = __builtin_inff();

  for (int base = 0; base < R; base += BC_KNN_TILE) {
    const int n = min(BC_KNN_TILE, R - base);  // rows past R: no candidates
    __syncthreads();  // the previous tile has been scanned by every wave
    for (int i = tid; i < n; i += 256)
      tile[i] = reinterpret_cast<const float4*>(archive)[base + i];
    __syncthreads();
    for (int r = 0; r < n; ++r) {
      const float4 a = tile[r];
      const float d0 = qv.x - a.x;
      const float d1 = qv.y - a.y;
      const float d2 = qv.z - a.z;
      const float d3 = qv.w - a.w;
      float acc = d0 * d0;
      acc = fmaf(d1, d1, acc);
      acc = fmaf(d2, d2, acc);
      acc = fmaf(d3, d3, acc);
      if (acc < best[BC_KNN_MAX - 1]) {
        // best[] ascending.  With p the first slot whose value exceeds
        // acc: slots above p take their lower neighbour, slot p takes acc,
        // slots below stay -- for every j that is the middle one of
        // (best[j-1], acc, best[j]), read before slot j-1 is rewritten.
#pragma unroll
        for (int j = BC_KNN_MAX - 1; j > 0; --j)
          best[j] = fminf(fmaxf(best[j - 1], acc), best[j]);
        best[0] = fminf(acc, best[0]);
      }
    }
  }

  if (!live) return;  // past the last barrier
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < BC_KNN_MAX; ++j) {
    if (j < k) {
      if (knn_d2 != nullptr) knn_d2[(size_t)q * k + j] = best[j];
      sum += sqrtf(best[j]);  // ascending order, k - 1 rounded adds
    }
  }
  novelty[q] = sum / (float)k;
}
