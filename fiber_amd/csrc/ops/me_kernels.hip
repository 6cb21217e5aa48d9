// MAP-Elites kernels (Mouret & Clune, "Illuminating search spaces by mapping
// elites"): a grid over behaviour space with one elite per cell, kept on the
// device.  Each generation mutates elites drawn from the filled cells; a
// child replaces the occupant of the cell its behaviour falls in only if it
// is strictly fitter.
//
//   me_parents         parent_idx[pop], slot[pop]: member m mutates the elite
//                      of a uniformly drawn filled cell (the root row while
//                      the archive is empty)
//   ga_rollout_mlp_bc  ga_rollout_mlp + bc[pop][4]
//   me_assign          cell[pop], and the best child of every cell by a
//                      64-bit atomicMax
//   me_commit          winner[C], order[C + 1], the archive's fitness, BC
//                      and filled flags
//   me_compact         filled_idx[0..n_filled) ascending, n_filled
//
// The weights of the archive are materialised by ga_survivors
// (ga_kernels.hip) from order[]: see me_commit.
//
// The mutation of member m in generation g is ga_rollout_mlp's for slot m:
// fam_normal4(seed, g, m, jb, FAM_TAG_NOISE, 0u, z) under ga_mutate, and the
// order of two fitness values is ga_rank_key's.  Both come from ga_shared.h,
// the BC epilogue from bc_epilogue.h, so that ga_rollout_mlp_bc,
// ga_survivors and ga_decode cannot disagree on a bit.
//
// The shared device code of es_kernels.hip is included below without its
// kernels, as ga_kernels.hip and ns_kernels.hip do, and for the same reason:
// this is a translation unit of its own so that its instantiation of
// rollout_steps cannot move the register allocation of es_rollout_mlp and
// es_eval_matrix (profiles/es_population.md, profiles/map_elites.md).

#define ES_KERNELS_SHARED_ONLY
#include "es_kernels.hip"
#include "ga_shared.h"
#include "bc_epilogue.h"
#include "me_grid.h"

// Philox tag of the parent draw; 0x45530001..4 are noise, env, conv obs and
// the GA's parent draw.
#define FAM_TAG_ME_PARENT 0x45530005u

// Member m mutates the elite of cell filled_idx[floor(u * n_filled / 2^32)],
// u one Philox word, with the draw of its own slot.  n_filled is read from
// device memory; while it is 0 every member's parent is root_row.  Integer
// only (fiber_amd/es/map_elites_oracle.py: parents_exact).
extern "C" __global__ void me_parents(uint32_t seed, uint32_t gen, int pop,
                                      const int* __restrict__ filled_idx,
                                      const int* __restrict__ n_filled_ptr,
                                      int root_row,
                                      int* __restrict__ parent_idx,
                                      int* __restrict__ slot) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= pop) return;
  const uint32_t n_filled = (uint32_t)*n_filled_ptr;
  const fam_uint4 u =
      philox4x32_10(seed, gen, (uint32_t)m, 0u, FAM_TAG_ME_PARENT, 0u);
  parent_idx[m] =
      n_filled == 0u ? root_row : filled_idx[fam_mulhi(u.x, n_filled)];
  slot[m] = m;
}

// ga_rollout_mlp with a BC per member.  Arguments, policy fill, LDS init,
// step loop and the fitness / obs-stat epilogue are that kernel's, line for
// line; only the last call is new, as in es_rollout_mlp_bc.
extern "C" __global__ void __launch_bounds__(256, ROLLOUT_WAVES)
ga_rollout_mlp_bc(const float* __restrict__ parents,   // [T][NPARAMS]
                  const int* __restrict__ parent_idx,  // [pop]
                  const int* __restrict__ slot,        // [pop]
                  float sigma, uint32_t seed, uint32_t gen, int horizon,
                  const float* __restrict__ obs_mu,
                  const float* __restrict__ obs_nu,
                  const float* __restrict__ env_A,    // [OBS][OBS]
                  const float* __restrict__ env_B,    // [OBS]
                  float* __restrict__ fitness,        // [pop]
                  float* __restrict__ obs_stat_part,  // [pop][2*OBS]
                  float* __restrict__ obs_stat_out,   // [2*OBS+1]
                  float* __restrict__ bc,             // [pop][OBS]
                  float* __restrict__ final_states)   // [pop][ENVS][OBS]
                                                      // or null
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

  // ---- behaviour characterisation --------------------------------------
  bc_reduce_store(L, tid, horizon, bc + (size_t)blockIdx.x * OBS,
                  final_states != nullptr
                      ? final_states + (size_t)blockIdx.x * (ENVS * OBS)
                      : nullptr);
}

// ---------------------------------------------------------------------------
// Insertion: me_assign, then me_commit.
//
// The cell of a member.  Per dimension t = (bc_d - lo_d) * inv_d, a subtract
// and a multiply rounded once each (a subtract feeding a multiply is not a
// pattern any fused instruction covers; the intrinsics say so in the
// source), b_d = floor(t) clamped to [0, bins_d - 1] in floating point, so
// that an infinite t takes an edge bin without an out-of-range conversion.
// A NaN in the BC or in the fitness gives cell -1: never inserted.
//
// The best child of a cell is the maximum, over the children that land in
// it, of the 64-bit key
//   (ga_rank_key(fitness) << 32) | (0xFFFFFFFE - m):
// the fitter child, among equals the lower member index.  Every such key is
// non-zero (m <= 65535), so best[] starts from zeros, and a maximum does not
// depend on the order in which the candidates arrive: the result is the
// same whatever the scheduling.
// ---------------------------------------------------------------------------
#define ME_TIE_TOP 0xFFFFFFFEu

__device__ __forceinline__ int me_bin(float x, float lo, float inv,
                                      int bins) {
  const float t = __fmul_rn(__fsub_rn(x, lo), inv);
  const float tf = floorf(t);
  const float top = (float)(bins - 1);  // exact: bins <= 65534
  if (!(tf > 0.f)) return 0;
  if (tf >= top) return bins - 1;
  return (int)tf;
}

extern "C" __global__ void me_assign(
    const float* __restrict__ fitness,  // [pop]
    const float* __restrict__ bc,       // [pop][4]
    int pop, MeGrid grid,
    int* __restrict__ cell,                  // [pop]
    unsigned long long* __restrict__ best)   // [C], zeroed
{
  static_assert(OBS == 4, "BC rows are read as float4");
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= pop) return;
  const float f = fitness[m];
  const float4 b = reinterpret_cast<const float4*>(bc)[m];
  if (f != f || b.x != b.x || b.y != b.y || b.z != b.z || b.w != b.w) {
    cell[m] = -1;
    return;
  }
  int c = me_bin(b.x, grid.lo[0], grid.inv[0], grid.bins[0]);
  c = c * grid.bins[1] + me_bin(b.y, grid.lo[1], grid.inv[1], grid.bins[1]);
  c = c * grid.bins[2] + me_bin(b.z, grid.lo[2], grid.inv[2], grid.bins[2]);
  c = c * grid.bins[3] + me_bin(b.w, grid.lo[3], grid.inv[3], grid.bins[3]);
  cell[m] = c;
  const unsigned long long key =
      ((unsigned long long)ga_rank_key(f) << 32) |
      (unsigned long long)(ME_TIE_TOP - (unsigned)m);
  atomicMax(&best[c], key);
}

// One thread per cell.  The best child displaces the occupant only if its
// key is strictly greater; an empty cell takes any child.  winner[c] = the
// member, or -1 where the cell is unchanged.  order[] is what ga_survivors
// needs to materialise the archive's weights out of place, with parent_idx
// and slot extended by C + 1 pseudo-members (member pop + c: parent c, slot
// -1): order[c] = the winner, or pop + c to copy the row as it is, and
// order[C] = pop + C, the root row.
extern "C" __global__ void me_commit(
    const float* __restrict__ fitness,            // [pop]
    const float* __restrict__ bc,                 // [pop][4]
    int pop, int C,
    const unsigned long long* __restrict__ best,  // [C]
    float* __restrict__ arch_fitness,             // [C]
    float* __restrict__ arch_bc,                  // [C][4]
    int* __restrict__ arch_filled,                // [C]
    int* __restrict__ winner,                     // [C]
    int* __restrict__ order)                      // [C + 1]
{
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > C) return;
  if (c == C) {
    order[C] = pop + C;
    return;
  }
  const unsigned long long key = best[c];
  bool take = key != 0ull;
  if (take && arch_filled[c] != 0)
    take = (unsigned)(key >> 32) > ga_rank_key(arch_fitness[c]);
  if (!take) {
    winner[c] = -1;
    order[c] = pop + c;
    return;
  }
  const int m = (int)(ME_TIE_TOP - (unsigned)(key & 0xFFFFFFFFull));
  winner[c] = m;
  order[c] = m;
  arch_fitness[c] = fitness[m];
  reinterpret_cast<float4*>(arch_bc)[c] =
      reinterpret_cast<const float4*>(bc)[m];
  arch_filled[c] = 1;
}

// filled_idx[0..n_filled) = the cells with arch_filled != 0, ascending;
// filled_idx[n_filled..C) = -1; *n_filled_out = their number.  One workgroup
// walks the cells in chunks of its size: a ballot and a popcount place a
// cell within its wave, the wave totals go through LDS, and the running base
// is carried in a register that every thread updates alike.
#define ME_COMPACT_THREADS 1024

extern "C" __global__ void __launch_bounds__(ME_COMPACT_THREADS)
me_compact(const int* __restrict__ arch_filled,  // [C]
           int C,
           int* __restrict__ filled_idx,    // [C]
           int* __restrict__ n_filled_out)  // [1]
{
  constexpr int WAVES = ME_COMPACT_THREADS / 64;
  __shared__ int wave_total[WAVES];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  int base = 0;
  for (int start = 0; start < C; start += ME_COMPACT_THREADS) {
    const int i = start + tid;
    const bool flag = i < C && arch_filled[i] != 0;
    const unsigned long long mask = __ballot(flag);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = __popcll(mask);
    __syncthreads();
    int offset = 0, total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const int t = wave_total[w];
      offset += w < wave ? t : 0;
      total += t;
    }
    if (flag) filled_idx[base + offset + before] = i;
    base += total;
    __syncthreads();  // wave_total has been read by every wave
  }
  for (int i = base + tid; i < C; i += ME_COMPACT_THREADS) filled_idx[i] = -1;
  if (tid == 0) *n_filled_out = base;
}
