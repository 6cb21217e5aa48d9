// LSTM recurrent policy for the ES engine (gfx950): a gated cell 4 -> 64 -> 2
// with torch.nn.LSTMCell's convention (gate order i, f, g, o), rolled out for
// the whole horizon in one launch, one workgroup per population member.
//
//   i = sigmoid(W_ii x + W_hi h + b_i)      f = sigmoid(W_if x + W_hf h + b_f)
//   g = tanh   (W_ig x + W_hg h + b_g)      o = sigmoid(W_io x + W_ho h + b_o)
//   c' = f * c + i * g                      h' = o * tanh(c')
//   logits = W_out h' + b_out               action = (l1 > l0), a tie is 0
//
//   es_rollout_lstm   perturbed members, es_rollout_gru's contract plus the
//                     optional final cell state
//   lstm_policy_step  one cell step for b rows: serving and numerics
//
// Both inline lstm_cell, so a check of one covers the arithmetic of the other.
//
// Work split.  512 threads = 8 waves, 64 envs.  Wave w owns hidden rows
// 16 (w & 3) ..+15 of all four gates for the two 16-env column tiles of half
// w >> 2.  A fourth gate does not fit gru_cell's split (one wave, four
// tiles): there the carried state alone would be 16 VGPRs per state.  Here
// the cell state is 2 tiles x 4 values = 8 VGPRs per lane, the resident W_h
// A fragments are 4 gates x 2 K-tiles x 4 = 32, and the SIMD still carries 4
// waves (two blocks of 8 per CU).  Per column tile the B fragments of h (two
// K-tiles) and of x are read ONCE and feed all four gates: 12 MFMAs on 3
// B-side reads.  Every accumulator starts from its fp32 bias quad.
//
// W_h is born in registers.  A lane's A fragment is 8 k-consecutive weights
// of one row, and every W_h row starts at a multiple of 8 in theta: the
// fragment is two aligned Philox blocks, drawn from theta and Philox
// straight into the registers (lstm_load).  W_h has no LDS staging tile and
// nothing aliases the h buffers.  The two waves that share a row strip each
// draw it.  W_i (narrow fragments), the biases and W_out go through LDS, one
// Philox block per thread.
//
// Two states.  c is carried in fp32 registers in the C/D layout and is never
// rounded or stored during the horizon.  h is only ever read back through
// the matmul, so only bf16(h'), the next step's B operand, goes to LDS,
// double-buffered by step parity; the fp32 h' feeds the logits in the same
// epilogue and is kept only at the last step, in LDS, for final_hidden.
//
// Two barriers per step: the MFMA phase with its epilogue (gates, c', h',
// logits partials through logits_reduce_swap into lpart), a barrier, the
// action / env step / reward / statistics / next-x phase on the first 256
// threads as (env, d = wave), restated from rollout_steps with its fmaf forms
// and constants, and the second barrier.
//
// Rounding points are the GRU kernel's: weights to bf16 when staged or
// drawn, biases fp32, the normalised clamped observation to bf16, the MFMA
// reads bf16(h), the logits read fp32 h'.

#define ES_KERNELS_SHARED_ONLY
#include "es_kernels.hip"

#define LGATES 4  // i, f, g, o: torch's order

// flat theta layout: every block starts at a multiple of 4, every W_h row at
// a multiple of 8
#define LOFF_WI 0                                // W_i[4][64][4]
#define LOFF_WH (LGATES * HID * OBS)             // 1024   W_h[4][64][64]
#define LOFF_B (LOFF_WH + LGATES * HID * HID)    // 17408  b[4][64]
#define LOFF_WO (LOFF_B + LGATES * HID)          // 17664  W_out[2][64]
#define LOFF_BO (LOFF_WO + ACT * HID)            // 17792  b_out[2]
#define LSTM_NPARAMS (LOFF_BO + ACT)             // 17794
static_assert(LOFF_WH % 8 == 0 && LOFF_B % 4 == 0 && LOFF_WO % 4 == 0 &&
                  LOFF_BO % 4 == 0,
              "Philox blocks never straddle two parameter blocks");

#define LSTM_THREADS 512
#define LSTM_WAVES 4  // waves per SIMD: 128 VGPRs, two blocks of 8 waves per CU
#define LSTM_ENV_THREADS (ENVS * OBS)  // the env phase: (env, d)

#define LOG2E 0x1.715476p+0f

// gru_kernels.hip's sigmoid: rcp(1 + exp2(-a * log2e)).  exp2 overflow gives
// inf and rcp(inf) = 0; underflow gives rcp(1) = 1.
__device__ inline float fast_sigmoid(float a) {
  const float e = __builtin_amdgcn_exp2f(a * -LOG2E);
  return __builtin_amdgcn_rcpf(1.0f + e);
}

// offsets into LstmLds::small, in theta's order from LOFF_B on
#define LS_WO (LGATES * HID)
#define LS_BO (LS_WO + ACT * HID)

struct LstmLds {
  alignas(16) __hip_bfloat16 hb[2][ENVS][S2];  // B operand of h, by parity
  alignas(16) __hip_bfloat16 wi[LGATES][HID][S1];  // narrow A rows
  // b[4][64], W_out[2][64], b_out[2] as fp32.  W_out only passes through on
  // its way into registers; the bias quads are read once too.
  alignas(16) float small[LS_BO + ACT + 2];
  alignas(16) __hip_bfloat16 xb[ENVS][S1];
  alignas(16) __hip_bfloat16 zero16[8];  // narrow kgrp>0 fragments
  // env state (double-buffered); es_rollout_lstm_cartpole reads a row as one
  // 16-byte vector
  alignas(16) float S[2][ENVS][OBS];
  float lpart[4][ENVS][2];   // per-strip logits partials
  float ostat[2 * OBS + 1];
  // fp32 h' of the last step, for final_hidden / Hnew: kept here, not in
  // registers (8 VGPRs that the step loop does not have)
  alignas(16) float hfin[ENVS][HID];
};

typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

// One lane's loop-invariant operands: 32 VGPRs of W_h A fragments, 16 of
// biases, 4 of W_out (bf16 pairs, widened by a shift and a mask per use).
struct LstmRegs {
  // W_h fragments [gate][k-tile], as the halves they are drawn in (frag)
  u32x2 ahh[2 * LGATES * (HID / 32)];
  __device__ bf16x8 frag(int g, int kk) const {
    const int f = g * (HID / 32) + kk;
    return __builtin_bit_cast(
        bf16x8,
        __builtin_shufflevector(ahh[2 * f], ahh[2 * f + 1], 0, 1, 2, 3));
  }
  f32x4 bq[LGATES];
  uint32_t wop[4];  // rows drow..drow+3: bf16 (action 0 | action 1 << 16)
};

// threadIdx.x through a copy that the compiler cannot see through.  Each
// phase derives its lane, row and address values from a fresh one: computed
// from threadIdx.x itself they are hoisted to the top, stay live through the
// Philox fill and the step loop, and spill.
__device__ __forceinline__ int lstm_tid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

__device__ __forceinline__ uint32_t lstm_bf16_bits(float v) {
  // the bf16 value widened back to fp32 keeps its 16 bits on top
  return __float_as_uint(__bfloat162float(__float2bfloat16(v))) >> 16;
}

// theta[j0 .. j0+3] of this member, j0 a multiple of 4: one Philox block.
template <bool PERTURB>
__device__ __forceinline__ f32x4 lstm_block4(const float* __restrict__ theta,
                                             float sgn, uint32_t seed,
                                             uint32_t iter, uint32_t pair,
                                             int j0) {
  f32x4 v = *reinterpret_cast<const f32x4*>(&theta[j0]);
  if (PERTURB) {
    float z[4];
    fam_normal4(seed, iter, pair, (uint32_t)(j0 >> 2), FAM_TAG_NOISE, 0u, z);
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = fmaf(sgn, z[u], v[u]);
  }
  return v;
}

// Fill R and the LDS operands of the policy.  The 353 small blocks (256 rows
// of W_i, 64 of biases, 32 of W_out, b_out) are one per thread; W_h goes from
// global memory through Philox into the A fragments.  Also writes the K
// padding of xb and the zero fragment, and ends in a barrier.
template <bool PERTURB>
__device__ __forceinline__ void lstm_load(const float* __restrict__ theta,
                                          float sgn, uint32_t seed,
                                          uint32_t iter, uint32_t pair,
                                          LstmLds& L, LstmRegs& R) {
  {
    const int t = lstm_tid();
    if (t < LGATES * HID) {
      // row t of W_i: 4 weights and 4 zeros, the kgrp 0 k-slots
      const f32x4 w = lstm_block4<PERTURB>(theta, sgn, seed, iter, pair,
                                           LOFF_WI + t * OBS);
      union {
        __hip_bfloat16 b[8];
        bf16x8 v;
      } pk;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        pk.b[u] = __float2bfloat16(w[u]);
        pk.b[4 + u] = __float2bfloat16(0.f);
      }
      *reinterpret_cast<bf16x8*>(&L.wi[0][0][0] + t * S1) = pk.v;
      // and the K padding of xb, columns 4..7
      L.xb[t >> 2][OBS + (t & 3)] = __float2bfloat16(0.f);
    } else if (t < LGATES * HID + LS_BO / 4) {
      const int m0 = (t - LGATES * HID) * 4;
      *reinterpret_cast<f32x4*>(&L.small[m0]) = lstm_block4<PERTURB>(
          theta, sgn, seed, iter, pair, LOFF_B + m0);
    } else if (t == LGATES * HID + LS_BO / 4) {
      // b_out: theta ends two values into this block
      float z[4] = {0.f, 0.f, 0.f, 0.f};
      if (PERTURB)
        fam_normal4(seed, iter, pair, (uint32_t)(LOFF_BO >> 2), FAM_TAG_NOISE,
                    0u, z);
#pragma unroll
      for (int a = 0; a < ACT; ++a)
        L.small[LS_BO + a] = PERTURB ? fmaf(sgn, z[a], theta[LOFF_BO + a])
                                     : theta[LOFF_BO + a];
    } else if (t < LGATES * HID + LS_BO / 4 + 1 + 8) {
      L.zero16[t - (LGATES * HID + LS_BO / 4 + 1)] = __float2bfloat16(0.f);
    }
  }

  // W_h: fragment f = (gate, k-tile) is theta[W_h + gate * 4096 + row * 64 +
  // k0 .. + 7], two Philox blocks; half n = 2f + (0 | 1) is one.  The loop
  // stays rolled (one copy of the draw, one draw's registers live at a time)
  // and shifts the halves through the array, so that every index is a
  // constant and the array lives in registers: after 16 rounds half n sits
  // in ahh[n].
  {
    constexpr int NH = 2 * LGATES * (HID / 32);
    const int t = lstm_tid();
    const int strip = (t >> 6) & 3, lane = t & 63;
    const int j00 = LOFF_WH + (strip * 16 + (lane & 15)) * HID +
                    (lane >> 4) * 8;
#pragma unroll
    for (int n = 0; n < NH; ++n) R.ahh[n] = u32x2{0u, 0u};
#pragma unroll 1
    for (int n = 0; n < NH; ++n) {
      // n = gate * 4 + k-tile * 2 + half
      const f32x4 w = lstm_block4<PERTURB>(
          theta, sgn, seed, iter, pair,
          j00 + (n >> 2) * (HID * HID) + ((n >> 1) & 1) * 32 + (n & 1) * 4);
      u32x2 half;
      half.x = lstm_bf16_bits(w[0]) | (lstm_bf16_bits(w[1]) << 16);
      half.y = lstm_bf16_bits(w[2]) | (lstm_bf16_bits(w[3]) << 16);
#pragma unroll
      for (int i = 0; i + 1 < NH; ++i) R.ahh[i] = R.ahh[i + 1];
      R.ahh[NH - 1] = half;
    }
  }
  __syncthreads();

  const int t = lstm_tid();
  const int drow = ((t >> 6) & 3) * 16 + ((t & 63) >> 4) * 4;  // C/D rows
#pragma unroll
  for (int g = 0; g < LGATES; ++g)
    R.bq[g] = *reinterpret_cast<const f32x4*>(&L.small[g * HID + drow]);
  const f32x4 w0 = *reinterpret_cast<const f32x4*>(&L.small[LS_WO + drow]);
  const f32x4 w1 =
      *reinterpret_cast<const f32x4*>(&L.small[LS_WO + HID + drow]);
#pragma unroll
  for (int ri = 0; ri < 4; ++ri)
    R.wop[ri] = lstm_bf16_bits(w0[ri]) | (lstm_bf16_bits(w1[ri]) << 16);
}

// One cell step of this wave's 16 hidden rows (strip) for its two column
// tiles (half): reads x from xb and bf16(h) from hcur, updates the fp32 cell
// state c[tile] in place, writes bf16(h') to hnext[env][row], the fp32 h' to
// hfin[env][row] unless hfin is null (wave-uniform), and the logits partials
// of its 32 envs to lrow = lpart[strip].  No barrier inside; the caller
// separates hcur / hnext / lpart users.
//
// SKIP (es_rollout_lstm_cartpole): bit cc of the wave-uniform `tiles` says
// that column tile cc of this half still has a live environment.  A dead
// tile costs no MFMA, no transcendental and no store; c[cc] keeps its value
// and the pair-wide logits reduce gets zeros for it.
template <bool SKIP = false>
__device__ __forceinline__ void lstm_cell(
    const LstmRegs& R, const __hip_bfloat16 (*wi)[HID][S1],
    const __hip_bfloat16* __restrict__ xb, const __hip_bfloat16* zero16,
    const __hip_bfloat16* __restrict__ hcur,
    __hip_bfloat16* __restrict__ hnext, f32x4 (&c)[2],
    float* __restrict__ hfin, float (*lrow)[2], int strip, int half,
    int lane, int tiles = 3) {
  const int drow = strip * 16 + (lane >> 4) * 4;
  float p0[2], p1[2];
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
    if (SKIP && !((tiles >> cc) & 1)) {
      p0[cc] = 0.f;
      p1[cc] = 0.f;
      continue;
    }
    const int bcol = (half * 2 + cc) * 16 + (lane & 15);
    // three B-side reads feed twelve MFMAs
    const bf16x8 bx = *strip_frag_ptr<S1, true>(xb, zero16, bcol, 0, lane >> 4);
    const bf16x8 bh0 =
        *strip_frag_ptr<S2, false>(hcur, nullptr, bcol, 0, lane >> 4);
    const bf16x8 bh1 =
        *strip_frag_ptr<S2, false>(hcur, nullptr, bcol, 1, lane >> 4);
    // The fp32 bias quads have the C/D layout (rows drow..drow+3), so each
    // accumulator starts from its bias: no add in the epilogue.
    f32x4 acc[LGATES];
#pragma unroll
    for (int g = 0; g < LGATES; ++g) {
      bf16x8 ai[1];
      strip_load_a<KPAD, S1, true>(&wi[g][0][0], zero16, strip, lane, ai);
      acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ai[0], bx, R.bq[g], 0,
                                                       0, 0);
    }
#pragma unroll
    for (int g = 0; g < LGATES; ++g)
      acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(R.frag(g, 0), bh0,
                                                       acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < LGATES; ++g)
      acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(R.frag(g, 1), bh1,
                                                       acc[g], 0, 0, 0);
    union {
      __hip_bfloat16 b[4];
      unsigned long long u;
    } pk;
    float q0 = 0.f, q1 = 0.f;
    f32x4 hq;
#pragma unroll
    for (int ri = 0; ri < 4; ++ri) {
      const float ig = fast_sigmoid(acc[0][ri]);
      const float fg = fast_sigmoid(acc[1][ri]);
      const float gg = fast_tanh(acc[2][ri]);
      const float og = fast_sigmoid(acc[3][ri]);
      // one product and one fma, spelled out so that both kernels round alike
      const float cn = fmaf(fg, c[cc][ri], ig * gg);
      c[cc][ri] = cn;
      const float hn = og * fast_tanh(cn);
      hq[ri] = hn;
      pk.b[ri] = __float2bfloat16(hn);
      q0 = fmaf(__uint_as_float(R.wop[ri] << 16), hn, q0);
      q1 = fmaf(__uint_as_float(R.wop[ri] & 0xffff0000u), hn, q1);
    }
    *reinterpret_cast<unsigned long long*>(&hnext[bcol * S2 + drow]) = pk.u;
    if (hfin != nullptr)
      *reinterpret_cast<f32x4*>(&hfin[bcol * HID + drow]) = hq;
    p0[cc] = q0;
    p1[cc] = q1;
  }
  logits_reduce_swap(p0[0], p1[0], p0[1], p1[1], lrow, half * 2, lane);
}

// lstm_cartpole_kernels.hip includes this file with
// LSTM_KERNELS_SHARED_ONLY defined, for everything above without the
// kernels below (the arrangement of es_kernels.hip).
#ifndef LSTM_KERNELS_SHARED_ONLY

extern "C" __global__ void __launch_bounds__(LSTM_THREADS, LSTM_WAVES)
es_rollout_lstm(const float* __restrict__ theta, float sigma, uint32_t seed,
                uint32_t iter, int horizon, int member_offset,
                const float* __restrict__ obs_mu,
                const float* __restrict__ obs_nu,
                const float* __restrict__ env_A,    // [OBS][OBS]
                const float* __restrict__ env_B,    // [OBS]
                int obs_mask,                       // bit d: dim d is visible
                float* __restrict__ fitness,        // [pop_shard]
                float* __restrict__ obs_stat_part,  // [pop_shard][2*OBS]
                float* __restrict__ obs_stat_out,   // [2*OBS+1]
                float* __restrict__ final_state,    // [pop_shard][64][4] / null
                float* __restrict__ final_hidden,   // [pop_shard][64][64]/null
                float* __restrict__ final_cell)     // [pop_shard][64][64]/null
{
  __shared__ LstmLds L;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int member = member_offset + blockIdx.x;
  const uint32_t pair = (uint32_t)(member >> 1);
  const float sgn = (member & 1) ? -sigma : sigma;

  // env init state: member-independent, common random numbers
  if (tid < ENVS) {
    float z[4];
    fam_normal4(seed, iter, (uint32_t)tid, 0u, FAM_TAG_ENV, 0u, z);
#pragma unroll
    for (int d = 0; d < OBS; ++d) L.S[0][tid][d] = 0.3f * z[d];
  }
  if (tid < 2 * OBS + 1) L.ostat[tid] = 0.f;
  // h = c = 0 at the start of the episode: buffer 0 and the registers
  for (int idx = tid; idx < ENVS * (HID / 4); idx += LSTM_THREADS)
    *reinterpret_cast<unsigned long long*>(
        &L.hb[0][idx >> 4][(idx & 15) * 4]) = 0ull;
  for (int idx = tid; idx < ENVS * (HID / 4); idx += LSTM_THREADS)
    *reinterpret_cast<f32x4*>(&L.hfin[idx >> 4][(idx & 15) * 4]) =
        (f32x4){0.f, 0.f, 0.f, 0.f};
  f32x4 c[2];
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) c[cc] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ---- the perturbed policy: registers and LDS; ends in a barrier -------
  LstmRegs R;
  lstm_load<true>(theta, sgn, seed, iter, pair, L, R);

  // ---- the env phase's per-thread state, as in rollout_steps ------------
  // The first 256 threads are (env, d = wave).  dd is made visibly
  // wave-uniform so that the eight constants below sit in SGPRs; waves 4..7
  // load those of d = wave - 4 and never use them.
  const int env = tid & 63;
  const bool env_wave = wave < OBS;  // wave-uniform
  const int dd = __builtin_amdgcn_readfirstlane(tid >> 6) & (OBS - 1);
  float raccp = 0.f, psum = 0.f, psq = 0.f;
  const float mu_d = obs_mu[dd];
  const float rstd_d = rsqrtf(obs_nu[dd] + 1e-4f);
  float eA_d[OBS];
#pragma unroll
  for (int e = 0; e < OBS; ++e) eA_d[e] = env_A[dd * OBS + e];
  const float eB_d = env_B[dd];
  const float one_if_d0 = (dd == 0) ? 1.f : 0.f;
  const bool visible = (obs_mask >> dd) & 1;  // wave-uniform

  // prologue for t = 0: stats + normalised obs from the init state
  if (horizon > 0 && env_wave) {
    const float s = L.S[0][env][dd];
    psum += s;
    psq += s * s;
    const float x = (s - mu_d) * rstd_d;
    L.xb[env][dd] =
        __float2bfloat16(visible ? fminf(5.f, fmaxf(-5.f, x)) : 0.f);
  }

  for (int t = 0; t < horizon; ++t) {
    const int cur = t & 1;
    __syncthreads();
    // ---- gates, c', h', logits partials (MFMA, one phase) ---------------
    lstm_cell(R, L.wi, &L.xb[0][0], L.zero16, &L.hb[cur][0][0],
              &L.hb[cur ^ 1][0][0], c,
              t == horizon - 1 ? &L.hfin[0][0] : nullptr, L.lpart[wave & 3],
              wave & 3, wave >> 2, lane);
    __syncthreads();
    // ---- action, env step, reward, stats, next xb -----------------------
    if (env_wave) {
      const float l0 = L.small[LS_BO] + L.lpart[0][env][0] +
                       L.lpart[1][env][0] + L.lpart[2][env][0] +
                       L.lpart[3][env][0];
      const float l1 = L.small[LS_BO + 1] + L.lpart[0][env][1] +
                       L.lpart[1][env][1] + L.lpart[2][env][1] +
                       L.lpart[3][env][1];
      const float asign = (l1 > l0) ? 1.f : -1.f;
      float drive = 0.f;
#pragma unroll
      for (int e = 0; e < OBS; ++e)
        drive = fmaf(eA_d[e], L.S[cur][env][e], drive);
      const float snew =
          fmaf(0.08f, fast_tanh(drive), 0.97f * L.S[cur][env][dd]) +
          0.05f * eB_d * asign;
      L.S[cur ^ 1][env][dd] = snew;
      raccp += one_if_d0 - 0.1f * snew * snew;
      if (t < horizon - 1) {
        psum += snew;
        psq += snew * snew;
        const float x = (snew - mu_d) * rstd_d;
        L.xb[env][dd] =
            __float2bfloat16(visible ? fminf(5.f, fmaxf(-5.f, x)) : 0.f);
      }
    }
  }
  __syncthreads();

  // Everything below is addressed from a fresh opaque copy of tid (lstm_tid).
  const int etid = lstm_tid();
  const int elane = etid & 63, ewave = etid >> 6;

  // ---- optional outputs: never touch what fitness / stats read ----------
  if (final_state != nullptr && etid < LSTM_ENV_THREADS)
    final_state[((size_t)blockIdx.x * ENVS + elane) * OBS + ewave] =
        L.S[horizon & 1][elane][ewave];
  {
    const int drow = (ewave & 3) * 16 + (elane >> 4) * 4;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      // each lane reads back what it wrote itself
      const int e = ((ewave >> 2) * 2 + cc) * 16 + (elane & 15);
      const size_t at = ((size_t)blockIdx.x * ENVS + e) * HID + drow;
      if (final_hidden != nullptr)
        *reinterpret_cast<f32x4*>(&final_hidden[at]) =
            *reinterpret_cast<const f32x4*>(&L.hfin[e][drow]);
      if (final_cell != nullptr)
        *reinterpret_cast<f32x4*>(&final_cell[at]) = c[cc];
    }
  }

  // ---- epilogue: fitness + obs-stat reductions, as es_rollout_gru -------
  if (ewave < OBS) {
    L.lpart[ewave][elane][0] = raccp;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      psum += __shfl_down(psum, off, 64);
      psq += __shfl_down(psq, off, 64);
    }
    if (elane == 0) {
      L.ostat[ewave] = psum;
      L.ostat[OBS + ewave] = psq;
    }
  }
  __syncthreads();
  if (ewave == 0) {
    float r = L.lpart[0][elane][0] + L.lpart[1][elane][0] +
              L.lpart[2][elane][0] + L.lpart[3][elane][0];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) r += __shfl_down(r, off, 64);
    if (elane == 0) fitness[blockIdx.x] = r / (float)ENVS;
  }
  if (etid < 2 * OBS)
    obs_stat_part[(size_t)blockIdx.x * (2 * OBS) + etid] = L.ostat[etid];
  if (etid == 0)
    atomicAdd(&obs_stat_out[2 * OBS], (float)(ENVS * horizon));
}

// One cell step for rows [64 * blockIdx.x, +64) of X[b][4] (already
// normalised), H[b][64] and C[b][64]: logits[b][2], Hnew[b][64], Cnew[b][64].
// Tail rows past b compute on zeros and store nothing.
extern "C" __global__ void __launch_bounds__(LSTM_THREADS, LSTM_WAVES)
lstm_policy_step(const float* __restrict__ theta, const float* __restrict__ X,
                 const float* __restrict__ H, const float* __restrict__ C,
                 int batch, float* __restrict__ logits,
                 float* __restrict__ Hnew, float* __restrict__ Cnew) {
  __shared__ LstmLds L;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int strip = wave & 3, half = wave >> 2;
  const size_t row0 = (size_t)blockIdx.x * ENVS;

  if (tid < LSTM_ENV_THREADS) {
    const int e = tid & 63, d = tid >> 6;
    const size_t row = row0 + e;
    L.xb[e][d] =
        __float2bfloat16(row < (size_t)batch ? X[row * OBS + d] : 0.f);
  }
  // this lane's fp32 c in the C/D layout, and bf16(h) as the B operand
  const int drow = strip * 16 + (lane >> 4) * 4;
  f32x4 c[2];
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
    const int e = (half * 2 + cc) * 16 + (lane & 15);
    const size_t row = row0 + e;
    f32x4 h = (f32x4){0.f, 0.f, 0.f, 0.f};
    c[cc] = h;
    if (row < (size_t)batch) {
      h = *reinterpret_cast<const f32x4*>(&H[row * HID + drow]);
      c[cc] = *reinterpret_cast<const f32x4*>(&C[row * HID + drow]);
    }
    union {
      __hip_bfloat16 b[4];
      unsigned long long u;
    } pk;
#pragma unroll
    for (int ri = 0; ri < 4; ++ri) pk.b[ri] = __float2bfloat16(h[ri]);
    *reinterpret_cast<unsigned long long*>(&L.hb[0][e][drow]) = pk.u;
  }

  LstmRegs R;
  lstm_load<false>(theta, 0.f, 0u, 0u, 0u, L, R);  // ends in a barrier

  lstm_cell(R, L.wi, &L.xb[0][0], L.zero16, &L.hb[0][0][0], &L.hb[1][0][0], c,
            &L.hfin[0][0], L.lpart[strip], strip, half, lane);
  __syncthreads();

#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
    const int e = (half * 2 + cc) * 16 + (lane & 15);
    const size_t row = row0 + e;
    if (row < (size_t)batch) {
      // each lane reads back what it wrote itself
      *reinterpret_cast<f32x4*>(&Hnew[row * HID + drow]) =
          *reinterpret_cast<const f32x4*>(&L.hfin[e][drow]);
      *reinterpret_cast<f32x4*>(&Cnew[row * HID + drow]) = c[cc];
    }
  }
  if (tid < ENVS * ACT) {
    const int e = tid >> 1, a = tid & 1;
    const size_t row = row0 + e;
    if (row < (size_t)batch)
      logits[row * ACT + a] = L.small[LS_BO + a] + L.lpart[0][e][a] +
                              L.lpart[1][e][a] + L.lpart[2][e][a] +
                              L.lpart[3][e][a];
  }
}
#endif  // LSTM_KERNELS_SHARED_ONLY
