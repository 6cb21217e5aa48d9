// Wide feed-forward policies for the ES engine (gfx950): 4 -> H -> H -> 2
// with H = 128 or 256, tanh hidden layers, rolled out for the whole horizon
// in one launch, one workgroup per population member.
//
//   es_rollout_mlp_wide_{128,256}     es_rollout_mlp's contract plus the
//                                     optional final env state
//   mlp_policy_forward_wide_{128,256} logits for b pre-normalised rows
//
// Both inline wide_load / wide_layer1 / wide_layer2 / wide_logit, so a check
// of one covers the arithmetic of the other.
//
// theta layout, the 64-wide one generalised:
//   W1[H][4]  b1[H]  W2[H][H]  b2[H]  W3[2][H]  b3[2]     H*H + 8H + 2
// Every block starts at a multiple of 4 and every W2 row at a multiple of 8.
//
// Why a kernel of its own.  The 64-wide step loop stages W2 in LDS, pulls
// one 16-row strip per wave into registers and lets h1 take over the tile
// (ENVS == HID).  At H = 256 W2 is 128 KiB in bf16: it does not fit the LDS
// of a CU next to h1, and 4 waves cannot hold it in registers either.
//
// W2 is born in the MFMA registers.  A lane's A fragment of
// v_mfma_f32_16x16x32_bf16 is 8 k-consecutive weights of one row, and with
// the layout above that is exactly two aligned Philox blocks of theta: the
// lane reads its 8 theta values from global, draws its two fam_normal4s,
// forms theta +- sigma z, rounds to bf16 and keeps the fragment for the
// whole horizon.  W2 never touches LDS, nothing is broadcast and nothing
// aliases.  The 8H + 2 small parameters are drawn one block per thread into
// LDS instead (wide_load): W1 as narrow bf16 A rows and the bias quads are
// read from there in every step, because resident they do not fit the
// register budget next to W2; the W3 slice is pulled into registers once.
//
// Work split.  512 threads = 8 waves; wave w owns hidden rows
// [w H/8, (w+1) H/8) of both layers: NS = H/128 strips of 16 rows.  W2 is
// resident in 16 NS^2 VGPRs per lane (16 / 64).  Per step:
//   layer 1  the NS narrow A fragments and bias quads are read once; per
//            16-env tile one narrow B fragment of x feeds the NS strips;
//            bias-started accumulator, fast_tanh, bf16, one packed 8-byte
//            store per strip into h1[env][H + 8]
//   layer 2  per tile the H/32 B fragments of h1 (ds_read_b128) are read
//            once and feed the NS strips; the accumulators stay in
//            registers through fast_tanh and the dot with the lane's W3
//            slice; logits_reduce_swap folds the four 16-lane rows and
//            lpart[8][64][2] carries the eight wave partials
//   env      the first 256 threads as (env, d), restated from rollout_steps
//            with its fmaf forms and constants
// Three barriers per step, as in the 64-wide loop.
//
// Rounding points are the 64-wide kernel's: W1, W2, W3 to bf16, the clamped
// normalised observation to bf16, h1 to bf16, h2 fp32 and never stored,
// biases fp32.  The serving kernel keeps h2 in fp32 too, so act() and the
// rollout form the same logits bits for the same x.
//
// The shared device code of es_kernels.hip is included without its kernels,
// as gru_kernels.hip does: a translation unit of its own cannot move the
// register allocation of es_rollout_mlp.

#define ES_KERNELS_SHARED_ONLY
#include "es_kernels.hip"

#define WIDE_THREADS 512
#define WIDE_NWAVES 8

template <int H>
struct WideGeom {
  static_assert(H == 128 || H == 256, "wide policies are 128 or 256 wide");
  static constexpr int NS = H / 128;  // 16-row strips per wave
  static constexpr int NK = H / 32;   // k-steps of layer 2
  static constexpr int NF = NS * NK;  // W2 fragments per lane
  static constexpr int ROWS = H / WIDE_NWAVES;  // rows per wave
  static constexpr int SH = H + 8;    // h1 LDS stride (bf16): 16 B rows
  // flat theta offsets
  static constexpr int B1 = OBS * H;
  static constexpr int W2 = B1 + H;
  static constexpr int B2 = W2 + H * H;
  static constexpr int W3 = B2 + H;
  static constexpr int B3 = W3 + ACT * H;
  static constexpr int NP = B3 + ACT;
  static_assert(B1 % 4 == 0 && W2 % 8 == 0 && B2 % 4 == 0 && W3 % 4 == 0 &&
                    B3 % 4 == 0 && H % 8 == 0,
                "fragments and quads are whole Philox blocks");
};

// Waves per SIMD each width is compiled for.  A block is 2 waves per SIMD:
// 128 VGPRs (4) keep two blocks on a CU.  At H = 128 a bound of 8 (64 VGPRs)
// leaves the rollout kernel 12 bytes of scratch; under the looser bound of 6
// the allocator settles at 64 VGPRs without any (profiles/wide_mlp.md).
template <int H> struct WideWaves;
template <> struct WideWaves<128> { static constexpr int value = 6; };
template <> struct WideWaves<256> { static constexpr int value = 4; };

template <int H>
struct WideLds {
  alignas(16) __hip_bfloat16 h1[ENVS][WideGeom<H>::SH];  // B operand, layer 2
  alignas(16) __hip_bfloat16 xb[ENVS][S1];               // B operand, layer 1
  // What the kgrp > 0 lanes of a narrow fragment read: zeros at the four
  // tile offsets of xb, so that one base address per lane serves all tiles
  alignas(16) __hip_bfloat16 zeros[3 * 16 * S1 + 8];
  float S[2][ENVS][OBS];                 // env state (double-buffered)
  float lpart[WIDE_NWAVES][ENVS][2];     // per-wave logits partials
  float ostat[2 * OBS + 1];
  // W1 as narrow A rows: 4 weights and 4 zeros (the kgrp 0 k-slots)
  alignas(16) __hip_bfloat16 w1[H][S1];
  // b1[H], b2[H], W3[2][H], b3[2] as fp32.  W3 only passes through on its
  // way into registers (wide_load); the bias quads are read in every step.
  alignas(16) float small[4 * H + 4];
};

typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

// One lane's loop-invariant operands.
template <int H>
struct WideRegs {
  // W2 fragments [strip][k-step], as the halves they are drawn in (frag)
  u32x2 a2h[2 * WideGeom<H>::NF];
  __device__ bf16x8 frag(int f) const {
    return __builtin_bit_cast(
        bf16x8,
        __builtin_shufflevector(a2h[2 * f], a2h[2 * f + 1], 0, 1, 2, 3));
  }
  uint32_t w3p[WideGeom<H>::NS][4];  // bf16 (action 0 | action 1 << 16)
  float b3[ACT];
};

// theta[j0 .. j0+3] of this member, j0 a multiple of 4: one Philox block.
template <bool PERTURB>
__device__ __forceinline__ f32x4 wide_block4(const float* __restrict__ theta,
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

union WidePack8 {
  __hip_bfloat16 b[8];
  bf16x8 v;
  __device__ WidePack8() {}
};

// threadIdx.x through a copy that the compiler cannot see through.  Each
// phase of the kernels derives its lane, row and address values from a
// fresh one: computed from threadIdx.x itself they are hoisted to the top,
// stay live through the Philox fill and the step loop, and spill.
__device__ __forceinline__ int wide_tid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

__device__ __forceinline__ uint32_t wide_bf16_bits(float v) {
  // the bf16 value widened back to fp32 keeps its 16 bits on top
  return __float_as_uint(__bfloat162float(__float2bfloat16(v))) >> 16;
}

// Fill R for the rows of wave `wave`.  W2 goes from global memory through
// Philox straight into the A fragments.  The 8H + 2 small parameters (W1,
// b1, b2, W3, b3) are drawn one block per thread into L.small and read back
// as quads behind the barrier inside: drawn in place they would cost every
// lane 5 NS + 1 draws, each repeated by the 16 lanes of a row, and the
// registers of those draws next to the resident W2 do not fit the budget.
template <int H, bool PERTURB>
__device__ __forceinline__ void wide_load(const float* __restrict__ theta,
                                          float sgn, uint32_t seed,
                                          uint32_t iter, uint32_t pair,
                                          WideLds<H>& L, WideRegs<H>& R) {
  typedef WideGeom<H> G;

  // Block mb < H is row mb of W1; the next H blocks are b1, b2 and W3 in
  // theta's order, H * H further on from b2; block 2H is b3, where theta
  // ends after two values.
  for (int mb = wide_tid(); mb <= 2 * H; mb += WIDE_THREADS) {
    const int m0 = (mb - H) * 4;  // index into small
    const int j0 = mb * 4 + (mb < H + H / 4 ? 0 : H * H);
    if (mb < H) {
      const f32x4 w = wide_block4<PERTURB>(theta, sgn, seed, iter, pair, j0);
      WidePack8 pk;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        pk.b[u] = __float2bfloat16(w[u]);
        pk.b[4 + u] = __float2bfloat16(0.f);
      }
      *reinterpret_cast<bf16x8*>(&L.w1[mb][0]) = pk.v;
    } else if (mb < 2 * H) {
      *reinterpret_cast<f32x4*>(&L.small[m0]) =
          wide_block4<PERTURB>(theta, sgn, seed, iter, pair, j0);
    } else {
      float z[4] = {0.f, 0.f, 0.f, 0.f};
      if (PERTURB)
        fam_normal4(seed, iter, pair, (uint32_t)(j0 >> 2), FAM_TAG_NOISE, 0u,
                    z);
#pragma unroll
      for (int a = 0; a < ACT; ++a)
        L.small[m0 + a] =
            PERTURB ? fmaf(sgn, z[a], theta[j0 + a]) : theta[j0 + a];
    }
  }

  // W2: fragment f = (strip, k-step) is theta[W2 + row * H + k0 .. + 7],
  // two Philox blocks; half g = 2f + (0 | 1) is one.  The loop stays rolled
  // (one copy of the draw instead of 2 NF, and one draw's registers live at
  // a time) and shifts the halves through the array, so that every index is
  // a constant and the array lives in registers: after 2 NF rounds half g
  // sits in a2h[g].
  {
    const int tid = wide_tid();
    const int wave = tid >> 6, lane = tid & 63;
    // row of strip 0 in the A layout, first k of this lane's group
    const int j00 = G::W2 + (wave * G::ROWS + (lane & 15)) * H +
                    (lane >> 4) * 8;
#pragma unroll
    for (int g = 0; g < 2 * G::NF; ++g) R.a2h[g] = u32x2{0u, 0u};
#pragma unroll 1
    for (int g = 0; g < 2 * G::NF; ++g) {
      const int f = g >> 1;
      const int s = f / G::NK, kk = f % G::NK;
      const f32x4 w = wide_block4<PERTURB>(
          theta, sgn, seed, iter, pair,
          j00 + s * 16 * H + kk * 32 + (g & 1) * 4);
      u32x2 half;
      half.x = wide_bf16_bits(w[0]) | (wide_bf16_bits(w[1]) << 16);
      half.y = wide_bf16_bits(w[2]) | (wide_bf16_bits(w[3]) << 16);
#pragma unroll
      for (int i = 0; i + 1 < 2 * G::NF; ++i) R.a2h[i] = R.a2h[i + 1];
      R.a2h[2 * G::NF - 1] = half;
    }
  }
  __syncthreads();

  const int tid = wide_tid();
  const int wave = tid >> 6, lane = tid & 63, kgrp = lane >> 4;
#pragma unroll
  for (int s = 0; s < G::NS; ++s) {
    const int d = wave * G::ROWS + s * 16 + kgrp * 4;  // C/D rows d..d+3
    const f32x4 w30 = *reinterpret_cast<const f32x4*>(&L.small[2 * H + d]);
    const f32x4 w31 = *reinterpret_cast<const f32x4*>(&L.small[3 * H + d]);
#pragma unroll
    for (int ri = 0; ri < 4; ++ri)
      R.w3p[s][ri] = wide_bf16_bits(w30[ri]) | (wide_bf16_bits(w31[ri]) << 16);
  }
#pragma unroll
  for (int a = 0; a < ACT; ++a)
    // the same value in every lane: keep it in an SGPR
    R.b3[a] = __uint_as_float(__builtin_amdgcn_readfirstlane(
        __float_as_uint(L.small[4 * H + a])));
}

// The K-padding of xb (columns 4..7) and the shared zero fragment.
template <int H>
__device__ __forceinline__ void wide_init_pads(WideLds<H>& L, int tid) {
  if (tid < ENVS * (S1 - OBS))
    L.xb[tid / (S1 - OBS)][OBS + tid % (S1 - OBS)] = __float2bfloat16(0.f);
  if (tid < 3 * 16 * S1 + 8) L.zeros[tid] = __float2bfloat16(0.f);
}

// h1 = bf16(tanh(W1 x + b1)) for this wave's rows and all 64 envs.
template <int H>
__device__ __forceinline__ void wide_layer1(const WideRegs<H>& R,
                                            WideLds<H>& L, int wave,
                                            int lane) {
  typedef WideGeom<H> G;
  const int drow = wave * G::ROWS + (lane >> 4) * 4;
  // The bias quads (rows drow..drow+3: the C/D layout) are read from LDS in
  // every step: resident they cost 8 NS VGPRs that the budget does not have.
  f32x4 b1q[G::NS];
#pragma unroll
  for (int s = 0; s < G::NS; ++s)
    b1q[s] = *reinterpret_cast<const f32x4*>(&L.small[drow + s * 16]);
  // The narrow fragments carry data in the kgrp 0 lanes only; the others
  // read zeros, at the same constant offsets from their base.
  const bool k0 = (lane >> 4) == 0;
  const __hip_bfloat16* xbase = k0 ? &L.xb[lane & 15][0] : &L.zeros[0];
  const __hip_bfloat16* abase =
      k0 ? &L.w1[wave * G::ROWS + (lane & 15)][0] : &L.zeros[0];
  bf16x8 a1[G::NS];
#pragma unroll
  for (int s = 0; s < G::NS; ++s)
    a1[s] = *reinterpret_cast<const bf16x8*>(abase + s * 16 * S1);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int bcol = ct * 16 + (lane & 15);
    const bf16x8 bx =
        *reinterpret_cast<const bf16x8*>(xbase + ct * 16 * S1);
#pragma unroll
    for (int s = 0; s < G::NS; ++s) {
      // the accumulator starts from the bias
      const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a1[s], bx, b1q[s], 0, 0, 0);
      union {
        __hip_bfloat16 b[4];
        unsigned long long u;
      } pk;
#pragma unroll
      for (int ri = 0; ri < 4; ++ri)
        pk.b[ri] = __float2bfloat16(fast_tanh(acc[ri]));
      *reinterpret_cast<unsigned long long*>(&L.h1[bcol][drow + s * 16]) =
          pk.u;
    }
  }
}

// h2 = tanh(W2 h1 + b2) in registers, its dot with the lane's W3 slice, and
// the wave's logits partials into lpart[wave].
template <int H>
__device__ __forceinline__ void wide_layer2(const WideRegs<H>& R,
                                            WideLds<H>& L, int wave,
                                            int lane) {
  typedef WideGeom<H> G;
  const int drow = wave * G::ROWS + (lane >> 4) * 4;
  f32x4 b2q[G::NS];
#pragma unroll
  for (int s = 0; s < G::NS; ++s)
    b2q[s] = *reinterpret_cast<const f32x4*>(&L.small[H + drow + s * 16]);
#pragma unroll
  for (int cp = 0; cp < 4; cp += 2) {
    float p0[2], p1[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int bcol = (cp + c) * 16 + (lane & 15);
      f32x4 acc[G::NS];
#pragma unroll
      for (int s = 0; s < G::NS; ++s) acc[s] = b2q[s];
#pragma unroll
      for (int kk = 0; kk < G::NK; ++kk) {
        // one fragment read feeds the NS strips
        const bf16x8 bh = *reinterpret_cast<const bf16x8*>(
            &L.h1[bcol][kk * 32 + (lane >> 4) * 8]);
#pragma unroll
        for (int s = 0; s < G::NS; ++s)
          acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              R.frag(s * G::NK + kk), bh, acc[s], 0, 0, 0);
      }
      float q0 = 0.f, q1 = 0.f;
#pragma unroll
      for (int s = 0; s < G::NS; ++s) {
#pragma unroll
        for (int ri = 0; ri < 4; ++ri) {
          const float h2 = fast_tanh(acc[s][ri]);
          q0 = fmaf(__uint_as_float(R.w3p[s][ri] << 16), h2, q0);
          q1 = fmaf(__uint_as_float(R.w3p[s][ri] & 0xffff0000u), h2, q1);
        }
      }
      p0[c] = q0;
      p1[c] = q1;
    }
    logits_reduce_swap(p0[0], p1[0], p0[1], p1[1], L.lpart[wave], cp, lane);
  }
}

// logit a of env e from the eight wave partials, in wave order.
template <int H>
__device__ __forceinline__ float wide_logit(const WideLds<H>& L, float b3a,
                                            int e, int a) {
  float l = b3a;
#pragma unroll
  for (int w = 0; w < WIDE_NWAVES; ++w) l += L.lpart[w][e][a];
  return l;
}

template <int H>
__device__ __forceinline__ void wide_rollout(
    const float* __restrict__ theta, float sigma, uint32_t seed,
    uint32_t iter, int horizon, int member_offset,
    const float* __restrict__ obs_mu, const float* __restrict__ obs_nu,
    const float* __restrict__ env_A, const float* __restrict__ env_B,
    float* __restrict__ fitness, float* __restrict__ obs_stat_part,
    float* __restrict__ obs_stat_out, float* __restrict__ final_state) {
  __shared__ WideLds<H> L;
  const int member = member_offset + blockIdx.x;
  const uint32_t pair = (uint32_t)(member >> 1);
  const float sgn = (member & 1) ? -sigma : sigma;

  {
    const int tid = wide_tid();
    wide_init_pads(L, tid);
    // env init state: member-independent, common random numbers
    if (tid < ENVS) {
      float z[4];
      fam_normal4(seed, iter, (uint32_t)tid, 0u, FAM_TAG_ENV, 0u, z);
#pragma unroll
      for (int d = 0; d < OBS; ++d) L.S[0][tid][d] = 0.3f * z[d];
    }
    if (tid < 2 * OBS + 1) L.ostat[tid] = 0.f;
  }

  WideRegs<H> R;
  wide_load<H, true>(theta, sgn, seed, iter, pair, L, R);
  __syncthreads();

  const int tid = wide_tid();
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- the env phase's per-thread state, as in rollout_steps ------------
  // Waves 0..3 run it as (env, d = wave); d is wave-uniform, so the eight
  // constants below sit in SGPRs.  Waves 4..7 load dim wave - 4 and never
  // use it.
  const bool envw = wave < OBS;
  const int env = tid & 63;
  const int dd = wave & (OBS - 1);
  float raccp = 0.f, psum = 0.f, psq = 0.f;
  const float mu_d = obs_mu[dd];
  const float rstd_d = rsqrtf(obs_nu[dd] + 1e-4f);
  float eA_d[OBS];
#pragma unroll
  for (int e = 0; e < OBS; ++e) eA_d[e] = env_A[dd * OBS + e];
  const float eB_d = env_B[dd];
  const float one_if_d0 = (dd == 0) ? 1.f : 0.f;

  // prologue for t = 0: stats + normalised obs from the init state
  if (envw && horizon > 0) {
    const float s = L.S[0][env][dd];
    psum += s;
    psq += s * s;
    const float x = (s - mu_d) * rstd_d;
    L.xb[env][dd] = __float2bfloat16(fminf(5.f, fmaxf(-5.f, x)));
  }

  for (int t = 0; t < horizon; ++t) {
    const int cur = t & 1;
    __syncthreads();
    wide_layer1(R, L, wave, lane);
    __syncthreads();
    wide_layer2(R, L, wave, lane);
    __syncthreads();
    // ---- action, env step, reward, stats, next xb -----------------------
    if (envw) {
      const float l0 = wide_logit(L, R.b3[0], env, 0);
      const float l1 = wide_logit(L, R.b3[1], env, 1);
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
        L.xb[env][dd] = __float2bfloat16(fminf(5.f, fmaxf(-5.f, x)));
      }
    }
  }
  __syncthreads();

  // ---- epilogue: fitness + obs-stat reductions, as es_rollout_mlp -------
  const int etid = wide_tid();
  const int eenv = etid & 63, edd = etid >> 6;  // edd < OBS: an env thread
  if (edd < OBS) {
    if (final_state != nullptr)
      final_state[((size_t)blockIdx.x * ENVS + eenv) * OBS + edd] =
          L.S[horizon & 1][eenv][edd];
    L.lpart[edd][eenv][0] = raccp;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      psum += __shfl_down(psum, off, 64);
      psq += __shfl_down(psq, off, 64);
    }
    if (eenv == 0) {
      L.ostat[edd] = psum;
      L.ostat[OBS + edd] = psq;
    }
  }
  __syncthreads();
  if (edd == 0) {
    float r = L.lpart[0][eenv][0] + L.lpart[1][eenv][0] +
              L.lpart[2][eenv][0] + L.lpart[3][eenv][0];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) r += __shfl_down(r, off, 64);
    if (eenv == 0) fitness[blockIdx.x] = r / (float)ENVS;
  }
  if (etid < 2 * OBS)
    obs_stat_part[(size_t)blockIdx.x * (2 * OBS) + etid] = L.ostat[etid];
  // every block adds the same value, so the order cannot change the sum
  if (etid == 0) atomicAdd(&obs_stat_out[2 * OBS], (float)(ENVS * horizon));
}

// logits[b][2] for rows [64 * blockIdx.x, +64) of X[b][4] (already
// normalised).  Tail rows past b compute on zeros and store nothing.
template <int H>
__device__ __forceinline__ void wide_forward(const float* __restrict__ theta,
                                             const float* __restrict__ X,
                                             int batch,
                                             float* __restrict__ logits) {
  __shared__ WideLds<H> L;
  const size_t row0 = (size_t)blockIdx.x * ENVS;
  {
    const int tid = wide_tid();
    wide_init_pads(L, tid);
    if (tid < ENVS * OBS) {
      const int e = tid & 63, d = tid >> 6;
      const size_t row = row0 + e;
      L.xb[e][d] =
          __float2bfloat16(row < (size_t)batch ? X[row * OBS + d] : 0.f);
    }
  }
  WideRegs<H> R;
  wide_load<H, false>(theta, 0.f, 0u, 0u, 0u, L, R);
  __syncthreads();
  const int tid = wide_tid();
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  wide_layer1(R, L, wave, lane);
  __syncthreads();
  wide_layer2(R, L, wave, lane);
  __syncthreads();
  if (tid < ENVS * ACT) {
    const int e = tid >> 1, a = tid & 1;
    const size_t row = row0 + e;
    if (row < (size_t)batch)
      logits[row * ACT + a] = wide_logit(L, a ? R.b3[1] : R.b3[0], e, a);
  }
}

#define WIDE_KERNELS(H)                                                      \
  extern "C" __global__ void                                                 \
      __launch_bounds__(WIDE_THREADS, WideWaves<H>::value)                   \
          es_rollout_mlp_wide_##H(                                           \
              const float* __restrict__ theta, float sigma, uint32_t seed,   \
              uint32_t iter, int horizon, int member_offset,                 \
              const float* __restrict__ obs_mu,                              \
              const float* __restrict__ obs_nu,                              \
              const float* __restrict__ env_A, /* [OBS][OBS] */              \
              const float* __restrict__ env_B, /* [OBS] */                   \
              float* __restrict__ fitness,       /* [pop_shard] */           \
              float* __restrict__ obs_stat_part, /* [pop_shard][2*OBS] */    \
              float* __restrict__ obs_stat_out,  /* [2*OBS+1] */             \
              float* __restrict__ final_state) /* [pop_shard][64][4]/null */ \
  {                                                                          \
    wide_rollout<H>(theta, sigma, seed, iter, horizon, member_offset,        \
                    obs_mu, obs_nu, env_A, env_B, fitness, obs_stat_part,    \
                    obs_stat_out, final_state);                              \
  }                                                                          \
  extern "C" __global__ void                                                 \
      __launch_bounds__(WIDE_THREADS, WideWaves<H>::value)                   \
          mlp_policy_forward_wide_##H(const float* __restrict__ theta,       \
                                      const float* __restrict__ X,           \
                                      int batch,                             \
                                      float* __restrict__ logits) {          \
    wide_forward<H>(theta, X, batch, logits);                                \
  }

WIDE_KERNELS(128)
WIDE_KERNELS(256)
