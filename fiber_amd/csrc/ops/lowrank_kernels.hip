// Low-rank correlated perturbations: what sampling a population from
// N(theta, sigma^2 T T^t) with T = scale * I + dirs^t mix dirs needs and
// the isotropic kernels cannot do.  A member's perturbation is d = T z, with
// z the FAM_TAG_NOISE draw of its pair; d[j] depends on the whole of z
// through the J dot products dirs z, so the policy fill is a phase of its
// own in front of the step loop instead of one fma per parameter.
//
//   es_rollout_mlp_lowrank  es_rollout_mlp with theta[j] +- sigma * d[j]
//   es_perturb_lowrank      the same parameters, written out as fp32 rows
//
// The kernels know nothing of the algorithm that owns (dirs, mix, scale);
// fiber_amd/es/lmmaes.py derives them for LM-MA-ES.  mix is read as a lower
// triangle: b[k] = sum_{l <= k} mix[k][l] p[l].
//
// How lowrank_fill splits the work, for a 256-thread workgroup:
//
//   draw    thread t owns the parameter blocks jb = t, t + 256, ... (5 at
//           most, 20 floats), drawn once and kept in registers, which are
//           dead before the step loop starts.
//   pass 1  8 directions at a time: every thread accumulates its share of
//           p[k] = dirs[k] . z from 16-byte loads, coalesced along the
//           parameters (dirs, 535 KB at J = 29, is read by every block and
//           lives in L2).  The 8 partials are transposed and reduced inside
//           the wave: three halving exchanges (8 -> 4 -> 2 -> 1 values per
//           lane) and three butterflies, 10 lane moves for 8 sums where a
//           tree per value takes 48.  Lane l < 8 then holds the wave's sum
//           for direction k0 + bitrev3(l) and stores it to LDS.
//   mix     one barrier; in EVERY wave lane k < J adds the 4 wave sums in
//           wave order and forms b[k] over its row of mix.  The waves
//           compute the same bits, so b needs no second trip through LDS:
//   pass 2  b[k] is read out of lane k into a scalar register, and
//           d = scale * z + sum_k b[k] * dirs[k][j] runs over the registers
//           that held z.  Then the member's theta[j] + sgn * d goes to the
//           sink.
//
// Every sum has a fixed order and there are no float atomics: the same bits
// on every run.  The 512 B of LDS scratch may alias whatever the sink
// writes (the rollout passes the start of its RolloutLds, which does not
// grow): a second barrier separates the last scratch read from the first
// sink call.
//
// A row of dirs is NPARAMS = 4610 floats, 18440 B, so odd rows start 8 B
// off a 16-byte boundary: the loads are typed 8-byte aligned (one
// global_load_dwordx4 all the same; the hardware needs dword alignment
// only).  The last parameter block, 1152, holds parameters 4608 and 4609
// and nothing else: it is loaded as 8 bytes, so that the last row is not
// read past its end.
//
// The shared device code of es_kernels.hip is included below without its
// kernels, as snes_kernels.hip does and for the same reason: this is a
// translation unit of its own so that its instantiation of rollout_steps
// cannot move the register allocation of es_rollout_mlp and es_eval_matrix
// (profiles/lmmaes.md has this file's own resource usage).

#define ES_KERNELS_SHARED_ONLY
#include "es_kernels.hip"

#define LOWRANK_DIRS_MAX 32
#define LOWRANK_GROUP 8                      // directions per pass-1 round
#define LOWRANK_NBLK ((NPARAMS + 3) / 4)     // 1153 parameter blocks
#define LOWRANK_SLOTS ((LOWRANK_NBLK + 255) / 256)  // 5 per thread
#define LOWRANK_TAIL (NPARAMS - 4 * (LOWRANK_NBLK - 1))  // 2 floats

static_assert(LOWRANK_TAIL == 2, "the tail block is loaded as one f32x2");
static_assert((NPARAMS * 4) % 8 == 0, "rows of dirs are 8-byte aligned");
static_assert(4 * LOWRANK_DIRS_MAX * sizeof(float) <= sizeof(PolicyLds),
              "the scratch aliases the policy tile");

typedef f32x4 __attribute__((aligned(8))) f32x4_a8;

// Parameters 4*jb .. 4*jb+3 of one row of dirs for slot I of thread tid,
// jb = tid + 256 * I.  Slots 0 .. 3 lie inside the row for every thread;
// in the last slot the tail block's two missing values read as 0, and a
// block past the end as four.
template <int I>
__device__ __forceinline__ f32x4 lowrank_load(const float* __restrict__ row,
                                              int tid) {
  const int jb = tid + 256 * I;
  if (I < LOWRANK_SLOTS - 1 || jb < LOWRANK_NBLK - 1)
    return *reinterpret_cast<const f32x4_a8*>(row + 4 * jb);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (jb == LOWRANK_NBLK - 1) {
    const f32x2 t = *reinterpret_cast<const f32x2*>(row + 4 * jb);
    v.x = t.x;
    v.y = t.y;
  }
  return v;
}
static_assert(256 * (LOWRANK_SLOTS - 1) <= LOWRANK_NBLK - 1,
              "slots before the last never reach the tail block");

// acc + row . z over this thread's slots, one fma per parameter in slot
// order.
template <int I = 0>
__device__ __forceinline__ float lowrank_dot(const float* __restrict__ row,
                                             int tid,
                                             const f32x4 (&z)[LOWRANK_SLOTS],
                                             float acc) {
  if constexpr (I < LOWRANK_SLOTS) {
    const f32x4 m = lowrank_load<I>(row, tid);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = fmaf(m[u], z[I][u], acc);
    return lowrank_dot<I + 1>(row, tid, z, acc);
  } else {
    return acc;
  }
}

// z += bk * row over this thread's slots.
template <int I = 0>
__device__ __forceinline__ void lowrank_axpy(const float* __restrict__ row,
                                             int tid, float bk,
                                             f32x4 (&z)[LOWRANK_SLOTS]) {
  if constexpr (I < LOWRANK_SLOTS) {
    const f32x4 m = lowrank_load<I>(row, tid);
#pragma unroll
    for (int u = 0; u < 4; ++u) z[I][u] = fmaf(bk, m[u], z[I][u]);
    lowrank_axpy<I + 1>(row, tid, bk, z);
  }
}

// One halving exchange of the transpose-reduce: a lane whose `bit` is clear
// keeps v[0 .. H-1] and hands v[H .. 2H-1] to its partner, a lane whose bit
// is set the other way round; each adds what it receives.
template <int H>
__device__ __forceinline__ void lowrank_halve(float (&v)[LOWRANK_GROUP],
                                              int lane, int bit) {
  const bool hi = (lane & bit) != 0;
#pragma unroll
  for (int m = 0; m < H; ++m) {
    const float keep = hi ? v[m + H] : v[m];
    const float send = hi ? v[m] : v[m + H];
    v[m] = keep + __shfl_xor(send, bit, 64);
  }
}

// Perturbed parameters of one member into `sink(j, value)`, every j <
// NPARAMS exactly once.  blockDim.x must be 256; scratch is
// 4 * LOWRANK_DIRS_MAX floats of LDS.  0 <= J <= LOWRANK_DIRS_MAX; J = 0
// reads neither dirs nor mix, has no barrier, and gives d = scale * z.
template <class Sink>
__device__ __forceinline__ void lowrank_fill(
    const float* __restrict__ theta, float sgn, uint32_t seed, uint32_t iter,
    uint32_t pair, const float* __restrict__ dirs,  // [J][NPARAMS]
    const float* __restrict__ mix,                  // [J][J]
    float scale, int J, float* scratch, int tid, Sink sink) {
  const int lane = tid & 63;
  const int wave = tid >> 6;

  // ---- draw -------------------------------------------------------------
  // values past NPARAMS are set to 0, so that they add nothing to a dot
  // product
  f32x4 z[LOWRANK_SLOTS];
#pragma unroll
  for (int i = 0; i < LOWRANK_SLOTS; ++i) {
    const int jb = tid + 256 * i;
    float zz[4] = {0.f, 0.f, 0.f, 0.f};
    if (jb < LOWRANK_NBLK)
      fam_normal4(seed, iter, pair, (uint32_t)jb, FAM_TAG_NOISE, 0u, zz);
#pragma unroll
    for (int u = 0; u < 4; ++u) z[i][u] = (4 * jb + u < NPARAMS) ? zz[u] : 0.f;
  }

  float b = 0.f;  // lane k < J: b[k]
  if (J > 0) {
    // ---- pass 1: p = dirs z, 8 directions per round ---------------------
    for (int k0 = 0; k0 < J; k0 += LOWRANK_GROUP) {
      float part[LOWRANK_GROUP];
#pragma unroll
      for (int kk = 0; kk < LOWRANK_GROUP; ++kk) {
        part[kk] = 0.f;
        if (k0 + kk < J)  // block-uniform
          part[kk] = lowrank_dot(dirs + (size_t)(k0 + kk) * NPARAMS, tid, z,
                                 0.f);
      }
      lowrank_halve<4>(part, lane, 1);
      lowrank_halve<2>(part, lane, 2);
      lowrank_halve<1>(part, lane, 4);
      float s = part[0];
      s += __shfl_xor(s, 8, 64);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      // lane bit 0 chose between kk and kk + 4, bit 1 between kk and
      // kk + 2, bit 2 between kk and kk + 1
      const int kk = ((lane & 1) << 2) | (lane & 2) | ((lane >> 2) & 1);
      if (lane < LOWRANK_GROUP && k0 + kk < J)
        scratch[wave * LOWRANK_DIRS_MAX + k0 + kk] = s;
    }
    __syncthreads();
    // ---- mix: b = tril(mix) p, the same bits in every wave --------------
    if (lane < J) {
      for (int l = 0; l <= lane; ++l) {
        const float p = ((scratch[l] + scratch[LOWRANK_DIRS_MAX + l]) +
                         scratch[2 * LOWRANK_DIRS_MAX + l]) +
                        scratch[3 * LOWRANK_DIRS_MAX + l];
        b = fmaf(mix[lane * J + l], p, b);
      }
    }
    __syncthreads();  // the sink may overwrite the scratch from here on
  }

  // ---- pass 2: d = scale * z + dirs^t b, over z's registers --------------
#pragma unroll
  for (int i = 0; i < LOWRANK_SLOTS; ++i) z[i] = z[i] * scale;
  for (int k = 0; k < J; ++k) {
    const float bk = __uint_as_float(
        __builtin_amdgcn_readlane(__float_as_uint(b), k));
    lowrank_axpy(dirs + (size_t)k * NPARAMS, tid, bk, z);
  }
#pragma unroll
  for (int i = 0; i < LOWRANK_SLOTS; ++i) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = 4 * (tid + 256 * i) + u;
      // es_rollout_mlp's expression, one fma
      if (j < NPARAMS) sink(j, theta[j] + sgn * z[i][u]);
    }
  }
}

// es_rollout_mlp with a low-rank correlated perturbation.  Arguments, LDS
// init, step loop and the fitness / obs-stat epilogue are that kernel's,
// line for line; only the policy fill differs.  With J = 0 and scale = 1 it
// writes that kernel's bits (tests/gpu/test_lmmaes_gpu.py).
extern "C" __global__ void __launch_bounds__(256, ROLLOUT_WAVES)
es_rollout_mlp_lowrank(const float* __restrict__ theta, float sigma,
                       const float* __restrict__ dirs,  // [J][NPARAMS]
                       const float* __restrict__ mix,   // [J][J]
                       float scale, int J, uint32_t seed, uint32_t iter,
                       int horizon, int member_offset,
                       const float* __restrict__ obs_mu,
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
  const float sgn = (member & 1) ? -sigma : sigma;

  // ---- fill perturbed policy into LDS ---------------------------------
  // the scratch is the head of L.pol, which nothing has written yet
  lowrank_fill(theta, sgn, seed, iter, pair, dirs, mix, scale, J,
               reinterpret_cast<float*>(&L), tid,
               [](int j, float v) { store_param(&L.pol, j, v); });
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

// The parameters es_rollout_mlp_lowrank rolls out, as fp32 rows (before the
// bf16 rounding of the weights): one workgroup per member, out[blockIdx.x]
// is member member_offset + blockIdx.x.
extern "C" __global__ void __launch_bounds__(256)
es_perturb_lowrank(const float* __restrict__ theta, float sigma,
                   const float* __restrict__ dirs,  // [J][NPARAMS]
                   const float* __restrict__ mix,   // [J][J]
                   float scale, int J, uint32_t seed, uint32_t iter,
                   int member_offset,
                   float* __restrict__ out)  // [n_members][NPARAMS]
{
  __shared__ float scratch[4 * LOWRANK_DIRS_MAX];
  const int member = member_offset + blockIdx.x;
  const float sgn = (member & 1) ? -sigma : sigma;
  float* __restrict__ row = out + (size_t)blockIdx.x * NPARAMS;
  lowrank_fill(theta, sgn, seed, iter, (uint32_t)(member >> 1), dirs, mix,
               scale, J, scratch, threadIdx.x,
               [row](int j, float v) { row[j] = v; });
}
