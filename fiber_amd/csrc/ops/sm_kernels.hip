// Safe mutations through output gradients for the Deep GA (Lehman et al.,
// "Safe Mutations for Deep and Recurrent Neural Networks through Output
// Gradients", SM-G): every weight's mutation step is sigma over the
// sensitivity of the policy's two logits to that weight, measured on a fixed
// batch of 64 probe states.
//
//   sm_steps           steps[T][NPARAMS] (and sens[T][NPARAMS]) of T parent
//                      rows: one forward and one backward pass per row
//   ga_rollout_mlp_sm  ga_rollout_mlp with a step row per parent
//   ga_survivors_sm    ga_survivors with the same step rows; one generation
//                      of a seed-chain decode is one call of it
//
// sm_steps, per parent row t (one workgroup, nothing shared between rows):
//   g_k(b)[j] = d logit_k(probe[b]) / d theta[j],  k = 0, 1, b = 0..63
//   abs mode   m_k[j] = (1/64) sum_b |g_k(b)[j]|
//   sum mode   m_k[j] = (1/64) sum_b  g_k(b)[j]
//   sens[j]  = sqrtf(fmaf(m_1, m_1, m_0 * m_0))
//   steps[j] = sigma / fmaxf(sens[j], s_min)        (IEEE fp32 division)
//
// Forward.  mlp_policy_forward's: the policy staged by store_param, the probe
// rounded to bf16 into xb, both layers through strip_mfma and
// fast_tanh4_bias, h1 and h2 rounded to bf16.  The logits themselves are not
// formed: only h1, h2 and the weights enter the gradients.
//
// Backward, per output k (op = fabsf in abs mode, the identity in sum mode):
//   s2[b][i]  = 1 - h2^2             fp32, fmaf(-h2, h2, 1): one rounding
//   d2[b][i]  = bf16(w3[k][i] * s2)  fp32 product, then ONE bf16 rounding
//   P[b][j]   = sum_i d2[b][i] W2[i][j]            MFMA, K = 64 over units
//   s1[b][j]  = 1 - h1^2             fp32, as s2
//   d1[b][j]  = bf16(P * s1)         fp32 product, then ONE bf16 rounding
//   dW2[i][j] = sum_b op(d2[b][i]) op(h1[b][j])    MFMA, K = 64 over batch
//   dW1[j][d] = sum_b op(d1[b][j]) op(x[b][d])     MFMA, K = 64 over batch
//   db2[i] = sum_b op(d2[b][i]),  db1[j] = sum_b op(d1[b][j]),
//   dW3[k][i] = sum_b op(h2[b][i])   fp32 adds in the VALU, b = 0..63 in order
//   dW3[1-k][i] = 0,  db3[k] = 64,  db3[1-k] = 0
// and m = sum * (1/64), exact.  |d * a| = |d| * |a|, so the abs reduction
// is the same GEMM on absolute values; op commutes with the bf16 rounding
// (a sign bit), so every operand is rounded once, signed, and op is applied
// where it is stored.  The signed d2 is what is back-propagated into P.
// These are all the bf16 roundings of the backward: d2 and d1.  s1, s2 and
// the products stay fp32; h1, h2, x, W2 are bf16 already.
//
// Where each operand is transposed.  strip_mfma reads A as [row][k] and B as
// [col][k] and leaves lane l with D[row = 4 (l >> 4) + r][col = l & 15] of
// its 16-row strip; the packed store of the four r goes to out[col][row..],
// i.e. transposed.  "Batch-major" is [b][unit], "feature-major" [unit][b].
//   W2      staged twice from global: pol.w2[i][j] (forward, store_param) and
//           w2t[j][i] (B of P: the sum runs over W2's ROW index)
//   x       staged twice: xb[b][d] (forward) and xT[d][b], op applied, rows
//           4..15 zero (B of dW1, one 16-column tile)
//   h1      layer-1 epilogue writes both h1[b][j] (packed store: B of layer
//           2) and h1T[j][b], op applied (scattered 2-byte stores: B of dW2;
//           the P epilogue squares it, so op does not matter there)
//   h2      never stored batch-major: s2 stays in registers, hT[i][b] =
//           op(h2) feeds the dW3 sums
//   d2      written from registers both ways: d2[b][i] signed (packed: A of
//           P, rows = batch) and d2T[i][b] = op(d2) (scattered: A of dW2)
//   d1      P has rows = batch, so the strip's own transposed packed store
//           writes d1T[j][b..b+3] = op(d1): A of dW1.  Never batch-major.
// LDS reuse (SmLds): d2 lives in pol.w2, d2T in h1, d1T in hT, each after a
// barrier behind the last read of what it replaces.
//
// Determinism.  No atomics.  Every sum is an MFMA or a fixed-order loop of
// one thread, every output element is written by exactly one thread, and a
// block reads its own row only: the result does not depend on T, on the
// row's position or on the launch shape.

#define ES_KERNELS_SHARED_ONLY
#include "es_kernels.hip"

// ga_mutate, shared with ga_kernels.hip and me_kernels.hip
#include "ga_shared.h"

#define SM_MODE_ABS 0
#define SM_MODE_SUM 1
#define SM_XT_ROWS 16  // one MFMA column tile; rows OBS..15 are zero

struct SmLds {
  PolicyLds pol;
  alignas(16) __hip_bfloat16 w2t[HID][S2];         // W2 transposed
  alignas(16) __hip_bfloat16 xb[ENVS][S1];         // probe, batch-major
  alignas(16) __hip_bfloat16 zero16[8];            // layer-1 kgrp>0 fragments
  alignas(16) __hip_bfloat16 xT[SM_XT_ROWS][S2];   // op(probe), feature-major
  alignas(16) __hip_bfloat16 h1[ENVS][S2];         // batch-major, signed
  alignas(16) __hip_bfloat16 h1T[HID][S2];         // op(h1), feature-major
  alignas(16) __hip_bfloat16 hT[HID][S2];          // op(h2), feature-major

  // W2 is read from pol.w2 only until the layer-2 A fragments are in
  // registers, h1 only by layer 2, hT only by the dW3 sums; the backward
  // writes its operands over them, after the barriers marked in sm_steps.
  __device__ __hip_bfloat16* d2() { return &pol.w2[0][0]; }  // [b][i]
  __device__ __hip_bfloat16* d2T() { return &h1[0][0]; }     // [i][b]
  __device__ __hip_bfloat16* d1T() { return &hT[0][0]; }     // [j][b]
};
static_assert(ENVS == HID, "the backward tiles are [64][S2] both ways");

// fabsf or the identity, as a mask on the sign bit (uniform over the launch)
__device__ __forceinline__ float sm_op(float v, unsigned keep) {
  return __uint_as_float(__float_as_uint(v) & keep);
}

// sum of one feature-major row over the batch, b = 0..63 in order
__device__ __forceinline__ float sm_row_sum(const __hip_bfloat16* row) {
  float s = 0.f;
  for (int b = 0; b < ENVS; ++b) s += __bfloat162float(row[b]);
  return s;
}

__device__ __forceinline__ unsigned long long sm_pack4(f32x4 v) {
  union {
    __hip_bfloat16 h[4];
    unsigned long long u;
  } pk;
#pragma unroll
  for (int ri = 0; ri < 4; ++ri) pk.h[ri] = __float2bfloat16(v[ri]);
  return pk.u;
}

__device__ __forceinline__ f32x4 sm_unpack4(unsigned long long u) {
  union {
    __hip_bfloat16 h[4];
    unsigned long long u;
  } pk;
  pk.u = u;
  f32x4 v;
#pragma unroll
  for (int ri = 0; ri < 4; ++ri) v[ri] = __bfloat162float(pk.h[ri]);
  return v;
}

// One parameter's sensitivity and step, written by the one thread that owns
// it.  sqrtf and the division are the correctly rounded ones (no fast-math).
__device__ __forceinline__ void sm_emit(float* __restrict__ srow,
                                        float* __restrict__ nrow, int j,
                                        float m0, float m1, float sigma,
                                        float s_min) {
  const float s = sqrtf(fmaf(m1, m1, m0 * m0));
  if (nrow != nullptr) nrow[j] = s;
  srow[j] = sigma / fmaxf(s, s_min);
}

extern "C" __global__ void __launch_bounds__(256)
sm_steps(const float* __restrict__ thetas,  // [T][NPARAMS]
         const float* __restrict__ probe,   // [ENVS][OBS]
         float sigma, float s_min, int mode,
         float* __restrict__ steps,         // [T][NPARAMS]
         float* __restrict__ sens)          // [T][NPARAMS] or null
{
  __shared__ SmLds L;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const unsigned keep = mode == SM_MODE_ABS ? 0x7FFFFFFFu : 0xFFFFFFFFu;
  const float* __restrict__ theta = thetas + (size_t)blockIdx.x * NPARAMS;

  // ---- stage the policy and the probe ----------------------------------
  for (int j = tid; j < NPARAMS; j += blockDim.x)
    store_param(&L.pol, j, theta[j]);
  for (int idx = tid; idx < HID * (S1 - OBS); idx += blockDim.x)
    L.pol.w1[idx / (S1 - OBS)][OBS + idx % (S1 - OBS)] =
        __float2bfloat16(0.f);
  for (int idx = tid; idx < HID * HID; idx += blockDim.x)
    L.w2t[idx & 63][idx >> 6] = __float2bfloat16(theta[OFF_W2 + idx]);
  for (int idx = tid; idx < ENVS * S1; idx += blockDim.x) {
    const int e = idx / S1, d = idx % S1;
    L.xb[e][d] = __float2bfloat16(d < OBS ? probe[e * OBS + d] : 0.f);
  }
  for (int idx = tid; idx < SM_XT_ROWS * ENVS; idx += blockDim.x) {
    const int d = idx >> 6, b = idx & 63;
    L.xT[d][b] =
        __float2bfloat16(d < OBS ? sm_op(probe[b * OBS + d], keep) : 0.f);
  }
  if (tid < 8) L.zero16[tid] = __float2bfloat16(0.f);
  __syncthreads();

  // this lane's strip rows drow..drow+3 and its column inside a tile
  const int drow = wave * 16 + (lane >> 4) * 4;
  const int lcol = lane & 15;

  // ---- forward, layer 1: h1 = bf16(tanh(W1 x + b1)) --------------------
  bf16x8 a1[KPAD / 32], a2[HID / 32];
  strip_load_a<KPAD, S1, true>(&L.pol.w1[0][0], L.zero16, wave, lane, a1);
  strip_load_a<HID, S2>(&L.pol.w2[0][0], nullptr, wave, lane, a2);
  const f32x4 b1q = strip_load_bias(L.pol.b1, wave, lane);
  const f32x4 b2q = strip_load_bias(L.pol.b2, wave, lane);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int bcol = ct * 16 + lcol;
    const f32x4 acc =
        strip_mfma<KPAD, S1, true>(a1, &L.xb[0][0], L.zero16, ct, lane);
    const f32x4 th = fast_tanh4_bias(acc, b1q);
    *reinterpret_cast<unsigned long long*>(&L.h1[bcol][drow]) = sm_pack4(th);
#pragma unroll
    for (int ri = 0; ri < 4; ++ri)
      L.h1T[drow + ri][bcol] = __float2bfloat16(sm_op(th[ri], keep));
  }
  __syncthreads();

  // ---- forward, layer 2: h2 = bf16(tanh(W2 h1 + b2)); s2 = 1 - h2^2 ----
  float s2[4][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int bcol = ct * 16 + lcol;
    const f32x4 acc =
        strip_mfma<HID, S2, false>(a2, &L.h1[0][0], nullptr, ct, lane);
    const f32x4 th = fast_tanh4_bias(acc, b2q);
#pragma unroll
    for (int ri = 0; ri < 4; ++ri) {
      const float h = __bfloat162float(__float2bfloat16(th[ri]));
      s2[ct][ri] = fmaf(-h, h, 1.f);
      L.hT[drow + ri][bcol] = __float2bfloat16(sm_op(h, keep));
    }
  }
  __syncthreads();  // pol.w2 and h1 are dead from here: d2 and d2T

  // dW3: thread i sums op(h2[.][i]) over the batch
  float m3 = 0.f;
  if (tid < HID) m3 = sm_row_sum(&L.hT[tid][0]) * (1.f / ENVS);

  // ---- backward, one output at a time ----------------------------------
  float g2[ACT][4][4];  // dW2[drow + ri][ct * 16 + lcol]
  float g1[ACT][4];     // dW1[drow + ri][lcol], lcol < OBS
  float gb2[ACT] = {0.f, 0.f}, gb1[ACT] = {0.f, 0.f};  // threads < HID
#pragma unroll
  for (int k = 0; k < ACT; ++k) {
    // d2 = bf16(w3[k] * s2), signed batch-major and op'd feature-major.
    // At k = 0 the barrier above is behind the last read of pol.w2, h1 and
    // (by this thread, just above) hT is only replaced after the next one;
    // at k = 1 the barrier that ends the loop body is.
    float w3r[4];
#pragma unroll
    for (int ri = 0; ri < 4; ++ri)
      w3r[ri] = __bfloat162float(L.pol.w3[k][drow + ri]);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int bcol = ct * 16 + lcol;
      f32x4 d;
#pragma unroll
      for (int ri = 0; ri < 4; ++ri) d[ri] = w3r[ri] * s2[ct][ri];
      *reinterpret_cast<unsigned long long*>(&L.d2()[bcol * S2 + drow]) =
          sm_pack4(d);
#pragma unroll
      for (int ri = 0; ri < 4; ++ri)
        L.d2T()[(drow + ri) * S2 + bcol] =
            __float2bfloat16(sm_op(d[ri], keep));
    }
    __syncthreads();

    // P[b][j] = sum_i d2[b][i] w2t[j][i]: strip rows are batch rows.
    // d1T[j][b..b+3] = op(bf16(P * (1 - h1^2))), the strip's transposed
    // packed store.  This is the first write over hT.
    {
      bf16x8 ad[HID / 32];
      strip_load_a<HID, S2>(L.d2(), nullptr, wave, lane, ad);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int jcol = ct * 16 + lcol;
        const f32x4 acc =
            strip_mfma<HID, S2, false>(ad, &L.w2t[0][0], nullptr, ct, lane);
        const f32x4 h = sm_unpack4(
            *reinterpret_cast<const unsigned long long*>(&L.h1T[jcol][drow]));
        f32x4 d;
#pragma unroll
        for (int ri = 0; ri < 4; ++ri) {
          const float s1 = fmaf(-h[ri], h[ri], 1.f);
          // op before the bf16 rounding or after it: the same value
          d[ri] = sm_op(acc[ri] * s1, keep);
        }
        *reinterpret_cast<unsigned long long*>(&L.d1T()[jcol * S2 + drow]) =
            sm_pack4(d);
      }
    }
    // dW2[i][j] = sum_b d2T[i][b] h1T[j][b]
    {
      bf16x8 at[HID / 32];
      strip_load_a<HID, S2>(L.d2T(), nullptr, wave, lane, at);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const f32x4 acc =
            strip_mfma<HID, S2, false>(at, &L.h1T[0][0], nullptr, ct, lane);
#pragma unroll
        for (int ri = 0; ri < 4; ++ri)
          g2[k][ct][ri] = acc[ri] * (1.f / ENVS);
      }
    }
    if (tid < HID) gb2[k] = sm_row_sum(&L.d2T()[tid * S2]) * (1.f / ENVS);
    __syncthreads();

    // dW1[j][d] = sum_b d1T[j][b] xT[d][b]: one column tile, d < OBS live
    {
      bf16x8 a3[HID / 32];
      strip_load_a<HID, S2>(L.d1T(), nullptr, wave, lane, a3);
      const f32x4 acc =
          strip_mfma<HID, S2, false>(a3, &L.xT[0][0], nullptr, 0, lane);
#pragma unroll
      for (int ri = 0; ri < 4; ++ri) g1[k][ri] = acc[ri] * (1.f / ENVS);
    }
    if (tid < HID) gb1[k] = sm_row_sum(&L.d1T()[tid * S2]) * (1.f / ENVS);
    __syncthreads();  // d2, d2T, d1T may be replaced
  }

  // ---- sens and steps: every parameter has one owner --------------------
  float* __restrict__ srow = steps + (size_t)blockIdx.x * NPARAMS;
  float* __restrict__ nrow =
      sens != nullptr ? sens + (size_t)blockIdx.x * NPARAMS : nullptr;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int ri = 0; ri < 4; ++ri)
      sm_emit(srow, nrow, OFF_W2 + (drow + ri) * HID + ct * 16 + lcol,
              g2[0][ct][ri], g2[1][ct][ri], sigma, s_min);
  if (lcol < OBS) {
#pragma unroll
    for (int ri = 0; ri < 4; ++ri)
      sm_emit(srow, nrow, OFF_W1 + (drow + ri) * OBS + lcol, g1[0][ri],
              g1[1][ri], sigma, s_min);
  }
  if (tid < HID) {
    sm_emit(srow, nrow, OFF_B1 + tid, gb1[0], gb1[1], sigma, s_min);
    sm_emit(srow, nrow, OFF_B2 + tid, gb2[0], gb2[1], sigma, s_min);
    // only output k reads W3 row k and b3[k]
    sm_emit(srow, nrow, OFF_W3 + tid, m3, 0.f, sigma, s_min);
    sm_emit(srow, nrow, OFF_W3 + HID + tid, 0.f, m3, sigma, s_min);
  }
  if (tid < ACT)
    sm_emit(srow, nrow, OFF_B3 + tid, tid == 0 ? 1.f : 0.f,
            tid == 0 ? 0.f : 1.f, sigma, s_min);
}

// ga_rollout_mlp with a step row per parent: member m with slot >= 0 fills
// ga_mutate(parent[j], steps[parent_idx[m]][j], z), the same explicit fma
// with the same draw; slot < 0 copies the row.  LDS init, step loop and
// epilogue are ga_rollout_mlp's, line for line.  parent_idx[m] must lie in
// [0, T) (not checked here).  The branch is uniform over the block.
extern "C" __global__ void __launch_bounds__(256, ROLLOUT_WAVES)
ga_rollout_mlp_sm(const float* __restrict__ parents,   // [T][NPARAMS]
                  const float* __restrict__ steps,     // [T][NPARAMS]
                  const int* __restrict__ parent_idx,  // [pop]
                  const int* __restrict__ slot,        // [pop]
                  uint32_t seed, uint32_t gen, int horizon,
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
  const size_t prow = (size_t)parent_idx[blockIdx.x] * NPARAMS;
  const float* __restrict__ theta = parents + prow;
  const float* __restrict__ step = steps + prow;
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
          store_param(&L.pol, j, ga_mutate(theta[j], step[j], z[u]));
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

// ga_survivors with a step row per parent: new_parents[t] = the weights
// member order[t] was evaluated with by ga_rollout_mlp_sm.  grid.x tiles the
// parameter blocks, grid.y is t.  Out of place: new_parents must alias
// neither parents nor steps.
extern "C" __global__ void ga_survivors_sm(
    const float* __restrict__ parents,   // [T_cur][NPARAMS]
    const float* __restrict__ steps,     // [T_cur][NPARAMS]
    const int* __restrict__ parent_idx,  // [pop]
    const int* __restrict__ slot,        // [pop]
    const int* __restrict__ order,       // [T]
    uint32_t seed, uint32_t gen,
    float* __restrict__ new_parents)     // [T][NPARAMS]
{
  const int jb = blockIdx.x * blockDim.x + threadIdx.x;
  if (jb * 4 >= NPARAMS) return;
  const int m = order[blockIdx.y];
  const size_t prow = (size_t)parent_idx[m] * NPARAMS;
  const float* __restrict__ theta = parents + prow;
  const float* __restrict__ step = steps + prow;
  const int sl = slot[m];
  float* __restrict__ row = new_parents + (size_t)blockIdx.y * NPARAMS;
  float z[4] = {0.f, 0.f, 0.f, 0.f};
  if (sl >= 0)
    fam_normal4(seed, gen, (uint32_t)sl, (uint32_t)jb, FAM_TAG_NOISE, 0u, z);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int j = jb * 4 + u;
    if (j < NPARAMS)
      row[j] = sl >= 0 ? ga_mutate(theta[j], step[j], z[u]) : theta[j];
  }
}
