// CartPole for the MLP ES engine: an environment with physics, failure and
// variable-length episodes on the MFMA rollout path.
//
//   es_rollout_mlp_cartpole  one workgroup of 256 threads per member, 64
//                            environments per member, the whole horizon in
//                            one launch
//   cartpole_stat_reduce     fixed-order sum of the per-member stat rows
//   cartpole_step            the same physics for states held by the caller
//
// The policy is es_rollout_mlp's 4 -> 64 -> 64 -> 2 MLP, filled from the
// same Philox counters (theta[j] + sgn * z), so es_grad and centered_rank
// serve this rollout unchanged.  The shared device code of es_kernels.hip
// is included below without its kernels; this file is a translation unit of
// its own like es_pairs_kernels.hip, and for the same reason.
//
// What differs from rollout_steps is the step loop:
//
// * Environment state in registers, replicated per wave.  Lane e of EVERY
//   wave holds the four state floats of environment e, its alive bit and
//   its step count.  The four waves run the same instructions on the same
//   inputs, so their copies are bit-identical; the state never goes to LDS
//   (no S[2][ENVS][OBS], no (env, dim) thread split).
// * live = __ballot(alive) is therefore the same 64-bit mask in all four
//   waves without any exchange, `if (live == 0) break;` is uniform across
//   the block, and the barrier count stays matched.
// * Compaction.  A live environment e presents its observation in row
//   slot(e) = popcount(live & ((1 << e) - 1)) of xb, and phases B and C run
//   only over the column tiles that hold live rows, in pairs (the swap
//   reduce works on tile pairs).  A column of D depends only on its column
//   of B, so an environment's logits do not depend on its slot: the result
//   is bit for bit that of an uncompacted loop.  Rows at or above nlive hold
//   stale finite values (xb starts zeroed) and are never read back.
//
// Arithmetic of the physics (cart_physics.h, shared with
// lstm_cartpole_kernels.hip): every fma and every separately rounded product
// is spelled out, so the compiler has no freedom in contraction.  Divisions
// are true IEEE divisions (__fdiv_rn), one per step; the divisions by
// mc + mp are products with a reciprocal formed once per launch.
// fiber_amd/es/cartpole_oracle.py reads it operation by operation.

#define ES_KERNELS_SHARED_ONLY
#include "es_kernels.hip"

// CartConst, cart_consts and cart_physics, shared with the LSTM kernel
#include "cart_physics.h"

// No state buffers: 14,112 B per block against RolloutLds' 16,208.
struct CartLds {
  PolicyLds pol;
  alignas(16) __hip_bfloat16 xb[ENVS][S1];  // compacted: row = slot
  alignas(16) __hip_bfloat16 zero16[8];
  float lpart[4][ENVS][2];                  // [wave][slot][action]

  // layer 2's B operand shares the W2 staging tile, as in RolloutLds: W2 is
  // only read from LDS before the step loop.
  __device__ __hip_bfloat16* h1() { return &pol.w2[0][0]; }
};

// Phase B for the tile pair (cp, cp + 1): mfma_strip_tanh_pre's body.
__device__ inline void cart_layer1_pair(const bf16x8 (&a1)[KPAD / 32],
                                        CartLds& L, f32x4 b1q, int cp,
                                        int wave, int lane) {
  __hip_bfloat16* __restrict__ h1 = L.h1();
  const int drow = wave * 16 + (lane >> 4) * 4;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int bcol = (cp + c) * 16 + (lane & 15);
    const f32x4 th = fast_tanh4_bias(
        strip_mfma<KPAD, S1, true>(a1, &L.xb[0][0], L.zero16, cp + c, lane),
        b1q);
    union {
      __hip_bfloat16 h[4];
      unsigned long long u;
    } pk;
#pragma unroll
    for (int ri = 0; ri < 4; ++ri) pk.h[ri] = __float2bfloat16(th[ri]);
    *reinterpret_cast<unsigned long long*>(&h1[bcol * S2 + drow]) = pk.u;
  }
}

// Phase C for the tile pair (cp, cp + 1): mfma_strip_logits' body, h2 in
// fp32 registers and the logits fused into the epilogue.
__device__ inline void cart_logits_pair(const bf16x8 (&a2)[HID / 32],
                                        CartLds& L, f32x4 b2q,
                                        const f32x2 (&w3p)[4], int cp,
                                        int wave, int lane) {
  f32x2 p[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const f32x4 h = fast_tanh4_bias(
        strip_mfma<HID, S2, false>(a2, L.h1(), nullptr, cp + c, lane), b2q);
    float p0 = 0.f, p1 = 0.f;
#pragma unroll
    for (int ri = 0; ri < 4; ++ri) {
      p0 = fmaf(w3p[ri].x, h[ri], p0);
      p1 = fmaf(w3p[ri].y, h[ri], p1);
    }
    p[c] = (f32x2){p0, p1};
  }
  logits_reduce_swap(p[0].x, p[0].y, p[1].x, p[1].y, L.lpart[wave], cp, lane);
}

#ifndef CARTPOLE_WAVES
#define CARTPOLE_WAVES 7
#endif

extern "C" __global__ void __launch_bounds__(256, CARTPOLE_WAVES)
es_rollout_mlp_cartpole(const float* __restrict__ theta, float sigma,
                        uint32_t seed, uint32_t iter, int horizon,
                        int member_offset, const float* __restrict__ obs_mu,
                        const float* __restrict__ obs_nu,
                        const float* __restrict__ cart,      // [8]
                        float* __restrict__ fitness,         // [pop]
                        float* __restrict__ stat_part,       // [pop][9]
                        int* __restrict__ lengths,           // [pop][64] / 0
                        float* __restrict__ final_state)     // [pop][64][4] / 0
{
  __shared__ CartLds L;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int member = member_offset + blockIdx.x;
  const uint32_t pair = (uint32_t)(member >> 1);
  const float sgn = (member & 1) ? -sigma : sigma;

  // ---- fill perturbed policy into LDS (es_rollout_mlp's) ----------------
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
  for (int idx = tid; idx < HID * (S1 - OBS); idx += blockDim.x)
    L.pol.w1[idx / (S1 - OBS)][OBS + idx % (S1 - OBS)] =
        __float2bfloat16(0.f);
  // all of xb: the K padding must be zero, and a row that no live
  // environment has written yet must be finite
  for (int idx = tid; idx < ENVS * S1; idx += blockDim.x)
    (&L.xb[0][0])[idx] = __float2bfloat16(0.f);
  if (tid < 8) L.zero16[tid] = __float2bfloat16(0.f);
  __syncthreads();

  f32x2 w3p[4];
  {
    const int drow = wave * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int ri = 0; ri < 4; ++ri) {
      w3p[ri].x = __bfloat162float(L.pol.w3[0][drow + ri]);
      w3p[ri].y = __bfloat162float(L.pol.w3[1][drow + ri]);
    }
  }
  // L.h1() is L.pol.w2: nothing reads W2 from LDS after the a2 load, and
  // the first h1 write of any wave comes after the loop-top barrier.
  bf16x8 a1[KPAD / 32], a2[HID / 32];
  strip_load_a<KPAD, S1, true>(&L.pol.w1[0][0], L.zero16, wave, lane, a1);
  strip_load_a<HID, S2>(&L.pol.w2[0][0], nullptr, wave, lane, a2);
  const f32x4 b1q = strip_load_bias(L.pol.b1, wave, lane);
  const f32x4 b2q = strip_load_bias(L.pol.b2, wave, lane);
  const float b30 = L.pol.b3[0], b31 = L.pol.b3[1];

  const CartConst k = cart_consts(cart);
  float mu[OBS], rstd[OBS];
#pragma unroll
  for (int d = 0; d < OBS; ++d) {
    mu[d] = obs_mu[d];
    rstd[d] = rsqrtf(obs_nu[d] + 1e-4f);
  }

  // ---- environment lane: the same in every wave --------------------------
  float s[OBS];
  {
    float z[4];
    fam_normal4(seed, iter, (uint32_t)lane, 0u, FAM_TAG_ENV, 0u, z);
#pragma unroll
    for (int d = 0; d < OBS; ++d) s[d] = 0.05f * z[d];
  }
  bool alive = true;
  int len = 0;
  // observation statistics: wave w keeps dimension w's lane partials, as
  // es_rollout_mlp does (two registers per lane where all four dimensions in
  // every wave would be eight)
  float psum = 0.f, psq = 0.f;

  for (int t = 0; t < horizon; ++t) {
    const unsigned long long live = __ballot(alive);
    if (live == 0) break;  // uniform across the block
    const int np = (__popcll(live) + 31) >> 5;  // tile pairs with live rows
    const int slot = __builtin_amdgcn_mbcnt_hi(
        (unsigned)(live >> 32),
        __builtin_amdgcn_mbcnt_lo((unsigned)live, 0u));
    // ---- phase A: statistics and the compacted observation row ----------
    if (alive) {
      union {
        __hip_bfloat16 h[4];
        unsigned long long u;
      } pk;
      const float sw = wave == 0 ? s[0] : wave == 1 ? s[1]
                       : wave == 2 ? s[2] : s[3];
      psum += sw;
      psq = fmaf(sw, sw, psq);
#pragma unroll
      for (int d = 0; d < OBS; ++d) {
        const float x = (s[d] - mu[d]) * rstd[d];
        pk.h[d] = __float2bfloat16(fminf(5.f, fmaxf(-5.f, x)));
      }
      if (wave == 0)
        *reinterpret_cast<unsigned long long*>(&L.xb[slot][0]) = pk.u;
    }
    __syncthreads();
    // ---- phase B: h1 = tanh(W1 x + b1) over the live tile pairs ----------
    cart_layer1_pair(a1, L, b1q, 0, wave, lane);
    if (np > 1) cart_layer1_pair(a1, L, b1q, 2, wave, lane);
    __syncthreads();
    // ---- phase C: logits --------------------------------------------------
    cart_logits_pair(a2, L, b2q, w3p, 0, wave, lane);
    if (np > 1) cart_logits_pair(a2, L, b2q, w3p, 2, wave, lane);
    __syncthreads();
    // ---- phase D: action and physics, in registers ------------------------
    if (alive) {
      const float l0 = b30 + L.lpart[0][slot][0] + L.lpart[1][slot][0] +
                       L.lpart[2][slot][0] + L.lpart[3][slot][0];
      const float l1 = b31 + L.lpart[0][slot][1] + L.lpart[1][slot][1] +
                       L.lpart[2][slot][1] + L.lpart[3][slot][1];
      const bool done = cart_physics(k, l1 > l0, s[0], s[1], s[2], s[3]);
      len += 1;  // the terminating step counts
      alive = !done;
    }
  }

  // ---- epilogue: a fixed shuffle tree per wave, no float atomics ----------
  float* __restrict__ row = stat_part + (size_t)blockIdx.x * CART_STATS;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    psum += __shfl_down(psum, off, 64);
    psq += __shfl_down(psq, off, 64);
  }
  if (lane == 0) {
    row[wave] = psum;
    row[OBS + wave] = psq;
  }
  if (wave != 0) return;
  if (lengths != nullptr) lengths[(size_t)blockIdx.x * ENVS + lane] = len;
  if (final_state != nullptr)
    *reinterpret_cast<f32x4*>(
        &final_state[((size_t)blockIdx.x * ENVS + lane) * OBS]) =
        (f32x4){s[0], s[1], s[2], s[3]};
  int total = len;  // exact: an integer sum, then one conversion
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    total += __shfl_down(total, off, 64);
  if (lane == 0) {
    fitness[blockIdx.x] = (float)total / (float)ENVS;
    row[2 * OBS] = (float)total;
  }
}

// obs_stat[c] = sum over members of part[m][c], c < 9 (the count rides in
// column 8): obs_stat_reduce's strided partials and LDS tree, one block per
// column, so the sum is the same every run.
extern "C" __global__ void __launch_bounds__(256)
cartpole_stat_reduce(const float* __restrict__ part, int nmembers,
                     float* __restrict__ obs_stat) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const int col = blockIdx.x;  // grid is exactly CART_STATS blocks
  float acc = 0.f;
  for (int m = tid; m < nmembers; m += 256)
    acc += part[(size_t)m * CART_STATS + col];
  red[tid] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) red[tid] += red[tid + st];
    __syncthreads();
  }
  if (tid == 0) obs_stat[col] = red[0];
}

// next_state[i], done[i] for state[i][4] and action[i] in {0, 1}: one thread
// per environment.  next_state may alias state.
extern "C" __global__ void __launch_bounds__(256)
cartpole_step(const float* state, const int* __restrict__ action,
              const float* __restrict__ cart, int n,
              float* next_state, int* __restrict__ done) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const CartConst k = cart_consts(cart);
  f32x4 s = *reinterpret_cast<const f32x4*>(&state[(size_t)i * OBS]);
  float x = s[0], xd = s[1], th = s[2], thd = s[3];
  done[i] = cart_physics(k, action[i] != 0, x, xd, th, thd) ? 1 : 0;
  *reinterpret_cast<f32x4*>(&next_state[(size_t)i * OBS]) =
      (f32x4){x, xd, th, thd};
}
