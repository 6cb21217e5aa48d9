// CDNA4 (gfx950) kernels for the ES engine — the hot path of the rebuild
// (SURVEY §2e kernel inventory: batched MLP policy forward on MFMA,
// obs-normalization in LDS, fitness/centered-rank reduction, on-the-fly
// Philox noise; reference workload: uber/fiber examples/gecco-2020/es.py).
//
// Design notes (MI355X-first):
// * es_rollout_mlp is a PERSISTENT kernel: one workgroup rolls out one
//   population member's E=64 synthetic-env episodes for the full horizon
//   T in a single launch — weights, activations and env state never leave
//   LDS, so the whole ES iteration is one kernel launch per rank plus one
//   tiny gradient launch (no per-step launch overhead, no HBM traffic for
//   activations).
// * Both matmul layers ride MFMA (v_mfma_f32_16x16x32_bf16): layer 1 is
//   K=32 (obs zero-padded 4->32), layer 2 is K=64.  A-operand = weights
//   [out][k] row-major in LDS; B-operand = activations [env][k] row-major
//   ("transposed" storage so each lane's 8 k-consecutive bf16 are one
//   ds_read_b128).
// * Perturbations are regenerated from Philox counters (philox.h), never
//   stored: member 2k applies +sigma*eps_k, member 2k+1 applies
//   -sigma*eps_k (antithetic pairs).
//
// Fragment layouts for v_mfma_f32_16x16x32_bf16 (A 16x32, B 32x16,
// C/D 16x16), per the CDNA4 guide + hardware verification test
// (tests/gpu/test_ops.py::test_mfma_gemm_against_torch):
//   A: lane l holds A[row=l&15][k=(l>>4)*8 + j], j=0..7
//   B: lane l holds B[k=(l>>4)*8 + j][col=l&15]
//   C/D: lane l, reg r holds D[row=(l>>4)*4 + r][col=l&15]

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include "philox.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

// tanh via the hardware transcendental unit (v_exp_f32):
// tanh(x) = 1 - 2/(e^{2x}+1).  ~6 VALU slots vs ~40 for libm tanhf —
// the rollout kernel evaluates 8192 activations per member-step, and the
// PMC profile (profiles/r01_rollout_pmc.md) showed the libm version made
// the kernel VALU-bound at 3.6% MfmaUtil.  exp overflow saturates
// correctly (inf -> tanh=1).
//
// e^{2x} = exp2(x * 2*log2(e)).  __expf(2x) lowers to v_mul(2x, log2e) +
// v_exp_f32; the doubling is folded into the constant instead: 2x is exact
// and 2*log2e is log2e with its exponent bumped (0x3fb8aa3b -> 0x4038aa3b),
// so both forms round the same real product — bit-identical, one VALU slot
// less per value (tests/test_tanh_fold.py).
#define TWO_LOG2E 0x1.715476p+1f  // bits 0x4038aa3b
__device__ inline float fast_tanh(float x) {
  float e = __builtin_amdgcn_exp2f(x * TWO_LOG2E);
  // v_rcp_f32 (1 inst, ~1 ulp) — plain division emits the full IEEE
  // v_div_scale/v_div_fmas chain (~10 insts), which dominated VALUBusy.
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

// 4-wide tanh(acc + bias) over one MFMA accumulator.  Only the
// quarter-rate v_exp/v_rcp are per-value; the rest of the chain — bias
// add, scale, +1, -2r+1 — is written on explicit 2-wide halves so that
// each link is one packed instruction per pair (v_pk_add / v_pk_mul /
// v_pk_fma: 8 plain VALU slots per call).  Left to the SLP vectoriser as
// f32x4 or scalar code the shape is fickle: folding the doubling into
// the constant un-packed the bias add in exchange (profiles/
// r04_rollout_issue_slots.md).
__device__ inline f32x2 tanh2_bias(f32x2 acc, f32x2 bias) {
  const f32x2 m = (acc + bias) * TWO_LOG2E;
  f32x2 e;
  e.x = __builtin_amdgcn_exp2f(m.x);
  e.y = __builtin_amdgcn_exp2f(m.y);
  const f32x2 ep1 = e + 1.0f;
  f32x2 r;
  r.x = __builtin_amdgcn_rcpf(ep1.x);
  r.y = __builtin_amdgcn_rcpf(ep1.y);
  return __builtin_elementwise_fma(r, (f32x2){-2.0f, -2.0f},
                                   (f32x2){1.0f, 1.0f});
}

__device__ inline f32x4 fast_tanh4_bias(f32x4 acc, f32x4 bias) {
  const f32x2 lo = tanh2_bias(acc.lo, bias.lo);
  const f32x2 hi = tanh2_bias(acc.hi, bias.hi);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
}

#define FAM_TAG_NOISE 0x45530001u
#define FAM_TAG_ENV 0x45530002u

// ---------------------------------------------------------------------------
// Policy geometry (compile-time; the flagship BASELINE config).
// ---------------------------------------------------------------------------
#define OBS 4
#define KPAD 32  // obs padded to one MFMA K-tile
#define HID 64
#define ACT 2
#define ENVS 64  // env instances per member (common random numbers)

// flat theta layout offsets
#define OFF_W1 0
#define OFF_B1 (HID * OBS)                  // 256
#define OFF_W2 (OFF_B1 + HID)               // 320
#define OFF_B2 (OFF_W2 + HID * HID)         // 4416
#define OFF_W3 (OFF_B2 + HID)               // 4480
#define OFF_B3 (OFF_W3 + ACT * HID)         // 4608
#define NPARAMS (OFF_B3 + ACT)              // 4610

// Layer-1 operands only carry 8 k-slots (obs 4 + 4 zeros): the MFMA is
// K=32, but the kgrp>0 lane groups feed all-zero fragments (one shared
// 16-byte LDS slot) instead of reading zero-padded tiles — identical
// math, and the w1/xb tiles shrink from 5 KB to 1 KB each (8 KB less LDS
// per block).  With h1 sharing the W2 staging tile (RolloutLds) the block
// is ~16 KB: LDS allows 10 workgroups/CU and no longer caps occupancy.
#define S1 8   // LDS stride (bf16) for layer-1 operands (16 B rows)
#define S2 72  // LDS stride (bf16) for K=64 operands

// One wave computes a 16-row strip of C[64][64] = A[64][K] x B[K][64],
// reading A as [row][k] (stride AS) and B as [col][k] (stride BS), then
// applies bias+tanh and stores C transposed into out[col][row] (stride OS)
// so the output is ready as the next layer's B-operand.
//
// NARROW=true: the operands carry only 8 real k-slots (obs 4 + 4 zero
// pad); the K=32 MFMA's kgrp>0 lane groups get all-zero fragments —
// bit-identical result, 1/4 the fragment LDS traffic, 1/4 the tile LDS.
// Those lanes read the zeros from `zero16`, one shared 16-byte slot of
// LDS zeros, through the same unconditional ds_read_b128 as the kgrp==0
// lanes read their row (a broadcast read): selecting the ADDRESS instead
// of the value needs no v_mov zeroing and no exec-mask toggling around
// the load, and the addresses are loop-invariant where the caller loops.
template <int S, bool NARROW>
__device__ inline const bf16x8* strip_frag_ptr(
    const __hip_bfloat16* __restrict__ M, const __hip_bfloat16* zero16,
    int row, int kk, int kgrp) {
  if (NARROW)
    return reinterpret_cast<const bf16x8*>(kgrp == 0 ? &M[row * S] : zero16);
  return reinterpret_cast<const bf16x8*>(&M[row * S + kk * 32 + kgrp * 8]);
}

// This lane's A fragments for its wave's 16-row strip, and its 4 bias
// values (rows drow..drow+3, drow = wave*16 + kgrp*4).  Both depend only
// on the policy, so a caller that loops over steps loads them once.
template <int K, int AS, bool NARROW = false>
__device__ inline void strip_load_a(const __hip_bfloat16* __restrict__ A,
                                    const __hip_bfloat16* zero16, int wave,
                                    int lane, bf16x8 (&afrag)[K / 32]) {
#pragma unroll
  for (int kk = 0; kk < K / 32; ++kk)
    afrag[kk] = *strip_frag_ptr<AS, NARROW>(A, zero16,
                                            wave * 16 + (lane & 15), kk,
                                            lane >> 4);
}

__device__ inline f32x4 strip_load_bias(const float* __restrict__ bias,
                                        int wave, int lane) {
  return *reinterpret_cast<const f32x4*>(
      &bias[wave * 16 + (lane >> 4) * 4]);
}

// acc for column tile ct of the strip (afrag from strip_load_a).
template <int K, int BS, bool NARROW>
__device__ inline f32x4 strip_mfma(const bf16x8 (&afrag)[K / 32],
                                   const __hip_bfloat16* __restrict__ B,
                                   const __hip_bfloat16* zero16, int ct,
                                   int lane) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < K / 32; ++kk) {
    const bf16x8 bfrag = *strip_frag_ptr<BS, NARROW>(
        B, zero16, ct * 16 + (lane & 15), kk, lane >> 4);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[kk], bfrag, acc, 0,
                                                  0, 0);
  }
  return acc;
}

template <int K, int BS, int OS, bool NARROW = false>
__device__ inline void mfma_strip_tanh_pre(
    const bf16x8 (&afrag)[K / 32], const __hip_bfloat16* __restrict__ B,
    const __hip_bfloat16* zero16, f32x4 biasq,
    __hip_bfloat16* __restrict__ out, int wave, int lane) {
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int bcol = ct * 16 + (lane & 15);
    const f32x4 acc = strip_mfma<K, BS, NARROW>(afrag, B, zero16, ct, lane);
    // D: row = r0 + kgrp*4 + ri, col = bcol.  The 4 rows are consecutive:
    // pack one 8-byte store into out[col][row..row+3].
    const int drow = wave * 16 + (lane >> 4) * 4;
    const f32x4 th = fast_tanh4_bias(acc, biasq);
    union {
      __hip_bfloat16 h[4];
      unsigned long long u;
    } pk;
#pragma unroll
    for (int ri = 0; ri < 4; ++ri) pk.h[ri] = __float2bfloat16(th[ri]);
    *reinterpret_cast<unsigned long long*>(&out[bcol * OS + drow]) = pk.u;
  }
}

// One-shot form (standalone forward / probe kernels): loads the A
// fragments and bias itself.  zero16 is only read when NARROW.
template <int K, int AS, int BS, int OS, bool NARROW = false>
__device__ inline void mfma_strip_tanh(const __hip_bfloat16* __restrict__ A,
                                       const __hip_bfloat16* __restrict__ B,
                                       const float* __restrict__ bias,
                                       __hip_bfloat16* __restrict__ out,
                                       int wave, int lane,
                                       const __hip_bfloat16* zero16 = nullptr) {
  bf16x8 afrag[K / 32];
  strip_load_a<K, AS, NARROW>(A, zero16, wave, lane, afrag);
  mfma_strip_tanh_pre<K, BS, OS, NARROW>(
      afrag, B, zero16, strip_load_bias(bias, wave, lane), out, wave, lane);
}

// Cross-kgrp reduce of the logits partials, for the column tiles ct and
// ct+1 at once.  Each lane holds its 4 rows' contribution to both logits
// of both tiles (p0 / p1 = logit 0 / 1); the sum over the wave's four
// 16-lane rows (kgrp 0..3) is one env's partial.  lrow = lpart[wave].
//
// Reference form: the shfl_xor tree, (k0+k1) + (k2+k3), through
// ds_bpermute, with the kgrp==0 lanes storing under an exec mask.  Only
// logits_reduce_probe uses it; the step loop runs the swap form below.
__device__ inline void logits_reduce_shfl(float p0, float p1,
                                          float (*lrow)[2], int ct,
                                          int lane) {
  p0 += __shfl_xor(p0, 16, 64);
  p1 += __shfl_xor(p1, 16, 64);
  p0 += __shfl_xor(p0, 32, 64);
  p1 += __shfl_xor(p1, 32, 64);
  if ((lane >> 4) == 0) {
    lrow[ct * 16 + lane][0] = p0;
    lrow[ct * 16 + lane][1] = p1;
  }
}

// Swap form: the same tree in the VALU.  Writing a register's four
// 16-lane rows as [r0 r1 r2 r3]:
//   v_permlane16_swap(x, y): x = [x0 y0 x2 y2], y = [x1 y1 x3 y3]
//   v_permlane32_swap(x, y): x = [x0 x1 y0 y1], y = [x2 x3 y2 y3]
// With p0 = [a0 a1 a2 a3], p1 = [b0 b1 b2 b3] of tile ct, one 16-swap and
// an add give s = [a0+a1, b0+b1, a2+a3, b2+b3]; tile ct+1 likewise gives
// t = [c0+c1, ...].  One 32-swap of (s, t) and an add give
// [a, b, c, d]: row kgrp holds logit kgrp&1 of tile ct + (kgrp>>1), each
// the sum (k0+k1) + (k2+k3) of the very operands the shfl tree adds —
// identical bits (tests/gpu/test_logits_reduce.py).  3 swaps + 3 adds per
// tile pair against 8 bpermutes + 8 adds, no LDS round trip to wait for,
// and the store is one unmasked full-wave ds_write.
__device__ inline f32x2 permlane16_swap(float x, float y) {
  const auto r = __builtin_amdgcn_permlane16_swap(
      __float_as_uint(x), __float_as_uint(y), false, false);
  return (f32x2){__uint_as_float(r[0]), __uint_as_float(r[1])};
}

__device__ inline f32x2 permlane32_swap(float x, float y) {
  const auto r = __builtin_amdgcn_permlane32_swap(
      __float_as_uint(x), __float_as_uint(y), false, false);
  return (f32x2){__uint_as_float(r[0]), __uint_as_float(r[1])};
}

__device__ inline void logits_reduce_swap(float p0a, float p1a, float p0b,
                                          float p1b, float (*lrow)[2],
                                          int ct, int lane) {
  const f32x2 sa = permlane16_swap(p0a, p1a);
  const f32x2 sb = permlane16_swap(p0b, p1b);
  const f32x2 s = permlane32_swap(sa.x + sa.y, sb.x + sb.y);
  const int kgrp = lane >> 4;
  lrow[(ct + (kgrp >> 1)) * 16 + (lane & 15)][kgrp & 1] = s.x + s.y;
}

// Layer-2 strip with the logits fused into the MFMA epilogue: the
// activations stay in fp32 registers (no bf16 pack / LDS store — they
// feed nothing but the logits), each lane accumulates its 4 rows'
// contribution to both action logits, and the reduce over the 4 kgrp lane
// groups yields the wave's per-env partial, written to lpart[wave][env].
// Removes the old D1 phase, its barrier, and all h2 LDS traffic.  w3p =
// this lane's 8 w3 weights: for each of its 4 rows the pair (action 0,
// action 1).
//
// The reduce runs on tile pairs (0,1) and (2,3) in the VALU
// (logits_reduce_swap): the first pair's swaps sit between the second
// pair's MFMAs and tanh chains, and no wave waits on LDS for a lane
// exchange.  The earlier ds_bpermute form had to stay per tile for that
// overlap — batching its permutes behind two waits measured 4.8% slower
// (profiles/r04_rollout_issue_slots.md); the swap form against it is in
// profiles/r05_rollout_occupancy.md.
template <int K, int BS>
__device__ inline void mfma_strip_logits(
    const bf16x8 (&afrag)[K / 32], const __hip_bfloat16* __restrict__ B,
    f32x4 biasq, const f32x2 (&w3p)[4], float (*lpart)[ENVS][2], int wave,
    int lane) {
#pragma unroll
  for (int cp = 0; cp < 4; cp += 2) {
    f32x2 p[2];  // {p0, p1} of tiles cp, cp+1
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const f32x4 acc =
          strip_mfma<K, BS, false>(afrag, B, nullptr, cp + c, lane);
      const f32x4 h = fast_tanh4_bias(acc, biasq);
      // Two scalar fma chains, 8 slots per tile.  While p0 / p1 fed
      // adjacent stores the compiler packed them (4 v_pk_fma); feeding the
      // swaps it does not.  Spelling the pair out as f32x2 fmas packs them
      // again but costs 6-9 VGPRs (below 7 waves/SIMD, or scratch) and
      // that build did not reproduce its own results across launch
      // shapes (profiles/r05_rollout_occupancy.md): keep the scalar form.
      float p0 = 0.f, p1 = 0.f;
#pragma unroll
      for (int ri = 0; ri < 4; ++ri) {
        p0 += w3p[ri].x * h[ri];
        p1 += w3p[ri].y * h[ri];
      }
      p[c] = (f32x2){p0, p1};
    }
    logits_reduce_swap(p[0].x, p[0].y, p[1].x, p[1].y, lpart[wave], cp,
                       lane);
  }
}

// Decompose flat theta index j -> LDS slot write.
struct PolicyLds {
  alignas(16) __hip_bfloat16 w1[HID][S1];
  alignas(16) __hip_bfloat16 w2[HID][S2];
  alignas(16) __hip_bfloat16 w3[ACT][HID];
  alignas(16) float b1[HID];  // read as f32x4 quads (strip_load_bias)
  alignas(16) float b2[HID];
  float b3[ACT];
};

__device__ inline void store_param(PolicyLds* p, int j, float v) {
  if (j < OFF_B1) {
    p->w1[j >> 2][j & 3] = __float2bfloat16(v);
  } else if (j < OFF_W2) {
    p->b1[j - OFF_B1] = v;
  } else if (j < OFF_B2) {
    int jj = j - OFF_W2;
    p->w2[jj >> 6][jj & 63] = __float2bfloat16(v);
  } else if (j < OFF_W3) {
    p->b2[j - OFF_B2] = v;
  } else if (j < OFF_B3) {
    int jj = j - OFF_W3;
    p->w3[jj >> 6][jj & 63] = __float2bfloat16(v);
  } else if (j < NPARAMS) {
    p->b3[j - OFF_B3] = v;
  }
}

// Shared epilogue/prologue state for one member rollout.
struct RolloutLds {
  PolicyLds pol;
  // layer-2 output never touches LDS (fused-logits epilogue keeps it in
  // registers), so only the layer-1 B operand and the layer-2 B operand
  // h1 live here — and h1 has no tile of its own, see h1() below.
  // 16,208 B per block: LDS allows 10 workgroups/CU, so the VGPR count
  // alone sets the occupancy.
  alignas(16) __hip_bfloat16 xb[ENVS][S1];
  alignas(16) __hip_bfloat16 zero16[8];     // layer-1 kgrp>0 fragments
  float S[2][ENVS][OBS];      // env state (double-buffered)
  float lpart[4][ENVS][2];  // per-wave logits partials (C -> D2)
  float ostat[2 * OBS + 1];   // sum, sumsq, count

  // B-operand of layer 2, [ENVS][S2].  It shares pol.w2 ([HID][S2], the
  // same shape: ENVS == HID): W2 is only staged there until rollout_steps
  // has pulled its A fragments into registers, which is before the step
  // loop; h1 is first written inside it.  This accessor is the one place
  // that knows; the invariant is spelled out where rollout_steps loads a2.
  __device__ __hip_bfloat16* h1() { return &pol.w2[0][0]; }
};
static_assert(ENVS == HID, "h1 [ENVS][S2] shares the W2 tile [HID][S2]");

// ---------------------------------------------------------------------------
// Pieces shared by es_rollout_mlp (perturbed members, obs statistics) and
// es_eval_matrix (explicit policies, no statistics).  Both kernels inline
// the SAME functions, so the step arithmetic cannot drift between them:
// at sigma = 0 the two produce bit-identical returns.  STATS compiles the
// obs-stat accumulation in (rollout) or out (eval).
// ---------------------------------------------------------------------------

// Everything in RolloutLds except the policy values: zero the K-padding of
// W1 (A-side zeros make pad products zero) and of xb, the shared zero
// fragment slot, draw the env init
// state (member-independent: common random numbers from seed, iter), zero
// the stat accumulators.  The caller fills L.pol and then barriers.
template <bool STATS>
__device__ __forceinline__ void rollout_init_lds(RolloutLds& L, int tid,
                                                 uint32_t seed,
                                                 uint32_t iter) {
  for (int idx = tid; idx < HID * (S1 - OBS); idx += blockDim.x) {
    L.pol.w1[idx / (S1 - OBS)][OBS + idx % (S1 - OBS)] =
        __float2bfloat16(0.f);
  }
  for (int idx = tid; idx < ENVS * (S1 - OBS); idx += blockDim.x) {
    L.xb[idx / (S1 - OBS)][OBS + idx % (S1 - OBS)] =
        __float2bfloat16(0.f);
  }
  if (tid < 8) L.zero16[tid] = __float2bfloat16(0.f);
  if (tid < ENVS) {
    float z[4];
    fam_normal4(seed, iter, (uint32_t)tid, 0u, FAM_TAG_ENV, 0u, z);
#pragma unroll
    for (int d = 0; d < OBS; ++d) L.S[0][tid][d] = 0.3f * z[d];
  }
  if (STATS) {
    if (tid < 2 * OBS + 1) L.ostat[tid] = 0.f;
  }
}

// The whole horizon for the policy in L.pol: prologue "phase A", then the
// B / C / D2 step loop, ending on the barrier that closes the last step.
// Call with L fully initialised and a barrier behind it.  Returns this
// thread's reward partial; with STATS, psum / psq receive its obs-stat
// partials.
//
// Every phase uses all 256 threads as (env = tid&63, d = tid>>6) —
// OBS==4 matches the 4 waves exactly.  The thread that owns (env, d)
// keeps its state component, obs-stat partials AND reward partial in
// REGISTERS across the whole horizon: phase A is folded into the tail
// of D2 (4 barriers per step), the fitness path stays deterministic
// (register partials, no float atomics), and only the cross-dim env
// state round-trips through LDS (for D2's drive term).
template <bool STATS>
__device__ __forceinline__ float rollout_steps(
    RolloutLds& L, int tid, int horizon, const float* obs_mu,
    const float* obs_nu,
    const float* env_A,  // [OBS][OBS]
    const float* env_B,  // [OBS]
    float& psum, float& psq) {
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int env = tid & 63;
  const int dd = tid >> 6;  // 0..3
  float raccp = 0.f;
  const float mu_d = obs_mu[dd];
  const float rstd_d = rsqrtf(obs_nu[dd] + 1e-4f);
  float eA_d[OBS];
#pragma unroll
  for (int e = 0; e < OBS; ++e) eA_d[e] = env_A[dd * OBS + e];
  const float eB_d = env_B[dd];
  const float one_if_d0 = (dd == 0) ? 1.f : 0.f;
  // this lane's w3 slice for the fused logits epilogue: rows
  // drow..drow+3 of both actions (drow = wave*16 + kgrp*4)
  f32x2 w3p[4];
  {
    const int drow = wave * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int ri = 0; ri < 4; ++ri) {
      w3p[ri].x = __bfloat162float(L.pol.w3[0][drow + ri]);
      w3p[ri].y = __bfloat162float(L.pol.w3[1][drow + ri]);
    }
  }

  // Loop-invariant MFMA operands, loaded once for the whole horizon: both
  // layers' A fragments (W1: 4 VGPRs, W2: 8) and bias quads (4 + 4).  LDS
  // no longer limits residency, so the VGPR count decides it: the kernels
  // must stay at <= 72 VGPRs (7 waves/SIMD) with these resident, and
  // without scratch.
  //
  // L.h1() is L.pol.w2.  That is sound because nothing reads W2 from LDS
  // after the a2 load below: every wave issues it here, the loop-top
  // __syncthreads() waits for the wave's outstanding LDS reads before it
  // arrives at the barrier, and the first h1 write of any wave (phase B)
  // comes after that barrier.  Do not read L.pol.w2 past this point.
  bf16x8 a1[KPAD / 32], a2[HID / 32];
  strip_load_a<KPAD, S1, true>(&L.pol.w1[0][0], L.zero16, wave, lane, a1);
  strip_load_a<HID, S2>(&L.pol.w2[0][0], nullptr, wave, lane, a2);
  const f32x4 b1q = strip_load_bias(L.pol.b1, wave, lane);
  const f32x4 b2q = strip_load_bias(L.pol.b2, wave, lane);

  // prologue "phase A" for t=0: stats + normalized obs from the init state
  {
    const float s = L.S[0][env][dd];
    if (STATS) {
      psum += s;
      psq += s * s;
    }
    float x = (s - mu_d) * rstd_d;
    L.xb[env][dd] = __float2bfloat16(fminf(5.f, fmaxf(-5.f, x)));
  }

  for (int t = 0; t < horizon; ++t) {
    const int cur = t & 1;
    __syncthreads();
    // ---- phase B: h1 = tanh(W1 x + b1)  (MFMA, K=32) ------------------
    mfma_strip_tanh_pre<KPAD, S1, S2, true>(a1, &L.xb[0][0], L.zero16, b1q,
                                            L.h1(), wave, lane);
    __syncthreads();
    // ---- phase C: h2 stays in registers; logits fused (MFMA, K=64) ----
    mfma_strip_logits<HID, S2>(a2, L.h1(), b2q, w3p, L.lpart, wave, lane);
    __syncthreads();
    // ---- phase D2 (+A of t+1): action, env step, stats, next xb -------
    {
      const float l0 = L.pol.b3[0] + L.lpart[0][env][0] +
                       L.lpart[1][env][0] + L.lpart[2][env][0] +
                       L.lpart[3][env][0];
      const float l1 = L.pol.b3[1] + L.lpart[0][env][1] +
                       L.lpart[1][env][1] + L.lpart[2][env][1] +
                       L.lpart[3][env][1];
      const float asign = (l1 > l0) ? 1.f : -1.f;
      // One fma per term, spelled out: left as `drive += a * s` the
      // compiler contracts all four or, with a different schedule around
      // it, multiplies two of them separately — other bits.
      float drive = 0.f;
#pragma unroll
      for (int e = 0; e < OBS; ++e)
        drive = fmaf(eA_d[e], L.S[cur][env][e], drive);
      // a*b + c*d leaves the compiler free to fuse either product into
      // the add, and the two choices round differently.  The fma is
      // spelled out (0.97*s rounded, 0.08*tanh fused) so that every
      // kernel that inlines this loop gets the same bits.
      const float snew =
          fmaf(0.08f, fast_tanh(drive), 0.97f * L.S[cur][env][dd]) +
          0.05f * eB_d * asign;
      L.S[cur ^ 1][env][dd] = snew;
      raccp += one_if_d0 - 0.1f * snew * snew;
      if (t < horizon - 1) {
        // next step's stats + normalized obs, from the register state
        if (STATS) {
          psum += snew;
          psq += snew * snew;
        }
        float x = (snew - mu_d) * rstd_d;
        L.xb[env][dd] = __float2bfloat16(fminf(5.f, fmaxf(-5.f, x)));
      }
    }
  }
  __syncthreads();
  return raccp;
}

// Reward epilogue, second half: wave 0, after every thread has staged its
// reward partial in L.lpart[dd][env][0] and the block has barriered.
// Lane e first forms env e's episode return from its 4 per-dim partials
// (stored to episodes[e] when that pointer is non-null), then a fixed
// shuffle tree sums the 64 returns — deterministic order.  The sum is
// valid in lane 0.
__device__ __forceinline__ float reward_reduce_wave0(
    const RolloutLds& L, int lane, float* __restrict__ episodes) {
  float r = L.lpart[0][lane][0] + L.lpart[1][lane][0] +
            L.lpart[2][lane][0] + L.lpart[3][lane][0];
  if (episodes != nullptr) episodes[lane] = r;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) r += __shfl_down(r, off, 64);
  return r;
}

// Waves per SIMD the two rollout kernels are compiled for (the second
// __launch_bounds__ argument: the register allocator and the scheduler
// then hold the kernel to 512 / ROLLOUT_WAVES VGPRs instead of trading a
// resident wave for a longer schedule).  LDS allows 10 blocks per CU.
#ifndef ROLLOUT_WAVES
#define ROLLOUT_WAVES 7
#endif

// Everything above is the shared device code of the MLP rollout kernels.
// es_pairs_kernels.hip includes this file with ES_KERNELS_SHARED_ONLY
// defined to get exactly that and none of the kernels below: the per-pair
// kernels are a translation unit of their own, so that the machine code
// of the two kernels here, 3 and 4 VGPRs under the 72 that 7 waves/SIMD
// allow, cannot depend on them: one more instantiation of rollout_steps
// in this module has moved their register allocation before
// (profiles/eval_matrix.md, profiles/es_population.md).
#ifndef ES_KERNELS_SHARED_ONLY

extern "C" __global__ void __launch_bounds__(256, ROLLOUT_WAVES)
es_rollout_mlp(const float* __restrict__ theta, float sigma, uint32_t seed,
               uint32_t iter, int horizon, int member_offset,
               const float* __restrict__ obs_mu,
               const float* __restrict__ obs_nu,
               const float* __restrict__ env_A,   // [OBS][OBS]
               const float* __restrict__ env_B,   // [OBS]
               float* __restrict__ fitness,       // [pop_shard]
               float* __restrict__ obs_stat_part, // [pop_shard][2*OBS]
               float* __restrict__ obs_stat_out)  // [2*OBS+1]
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

  // ---- epilogue: fitness + obs-stat reductions -------------------------
  // reward partials: 4 per env (one per dim-owner thread), staged via
  // lpart then wave-0 shuffle-reduced — deterministic order.
  L.lpart[dd][env][0] = raccp;
  // obs-stat partials: wave w holds dim w for all 64 envs, so a fixed
  // shuffle tree gives the same sum every run (no float atomics).
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

// K explicit (unperturbed) policies x M environments in one launch: one
// workgroup per cell.  The cell index is flattened into blockIdx.x
// (k = cell / M, m = cell % M) because gridDim.y stops at 65535 and K*M
// does not.  theta_k goes straight into LDS — no Philox, no add — and
// each policy brings its own obs normaliser; the env states and the
// step loop are es_rollout_mlp's (common random numbers from seed,
// iter), so scores[k][m] is bit-identical to that kernel's fitness for
// theta_k at sigma = 0.  No obs statistics, no atomics.
extern "C" __global__ void __launch_bounds__(256, ROLLOUT_WAVES)
es_eval_matrix(const float* __restrict__ thetas,  // [K][NPARAMS]
               const float* __restrict__ obs_mu,  // [K][OBS]
               const float* __restrict__ obs_nu,  // [K][OBS]
               const float* __restrict__ env_A,   // [M][OBS][OBS]
               const float* __restrict__ env_B,   // [M][OBS]
               uint32_t seed, uint32_t iter, int horizon, int M,
               float* __restrict__ scores,        // [K][M]
               float* __restrict__ episodes)      // [K][M][ENVS] or null
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
}

// obs_stat_out[c] = sum over members of part[m][c], c < 2*OBS: one block
// per column, strided partials then a fixed LDS tree — run-to-run
// reproducible, unlike float atomics from 32k blocks.
extern "C" __global__ void __launch_bounds__(256)
obs_stat_reduce(const float* __restrict__ part, int nmembers,
                float* __restrict__ obs_stat_out) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const int col = blockIdx.x;  // grid is exactly 2*OBS blocks
  float acc = 0.f;
  for (int m = tid; m < nmembers; m += 256)
    acc += part[(size_t)m * (2 * OBS) + col];
  red[tid] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) obs_stat_out[col] = red[0];
}

// ---------------------------------------------------------------------------
// Gradient: g[j] = sum_pairs w_k * eps_k[j]  (eps regenerated via Philox).
// grid.x tiles the parameter blocks, grid.y tiles the local pair range.
// ---------------------------------------------------------------------------
extern "C" __global__ void es_grad(const float* __restrict__ wpair,
                                   int pair_begin, int pair_end,
                                   int pairs_per_chunk, uint32_t seed,
                                   uint32_t iter, int nparams,
                                   float* __restrict__ out) {
  const int jb = blockIdx.x * blockDim.x + threadIdx.x;
  if (jb * 4 >= nparams) return;
  const int chunk_begin = pair_begin + blockIdx.y * pairs_per_chunk;
  const int chunk_end = min(chunk_begin + pairs_per_chunk, pair_end);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int pair = chunk_begin; pair < chunk_end; ++pair) {
    const float w = wpair[pair];
    if (w == 0.f) continue;
    float z[4];
    fam_normal4(seed, iter, (uint32_t)pair, (uint32_t)jb, FAM_TAG_NOISE, 0u,
                z);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] += w * z[u];
  }
  // Each (chunk, j) is written by exactly one thread.  With one chunk
  // `out` is the gradient itself; otherwise it is the [chunks][nparams]
  // partial buffer that es_grad_reduce sums in chunk order, so the result
  // is the same every run (no float atomics).
  float* __restrict__ row = out + (size_t)blockIdx.y * nparams;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int j = jb * 4 + u;
    if (j < nparams) row[j] = acc[u];
  }
}

extern "C" __global__ void es_grad_reduce(const float* __restrict__ part,
                                          int chunks, int nparams,
                                          float* __restrict__ grad) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nparams) return;
  float acc = 0.f;
  for (int c = 0; c < chunks; ++c) acc += part[(size_t)c * nparams + j];
  grad[j] = acc;
}

// ---------------------------------------------------------------------------
// Centered rank: out[i] = rank(f_i)/(n-1) - 0.5 with deterministic
// index-order tie-break.  O(n^2/threads) — n is the population (<=64k).
// ---------------------------------------------------------------------------
extern "C" __global__ void centered_rank(const float* __restrict__ f, int n,
                                         float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float fi = f[i];
  int rank = 0;
  for (int j = 0; j < n; ++j) {
    const float fj = f[j];
    rank += (fj < fi) || (fj == fi && j < i);
  }
  out[i] = (float)rank / (float)(n - 1) - 0.5f;
}

// ---------------------------------------------------------------------------
// Sort-based centered rank for large populations (>16k members, e.g. the
// named 8-GPU config at pop 131,072, where the O(n^2) kernel would cost
// milliseconds).  Keys are floats mapped to order-preserving uint32
// (sign-flip trick); a stable device radix sort (rocPRIM, driven from the
// host launcher) then yields rank = sorted position with the same
// index-order tie-break as torch.argsort(stable=True).
// ---------------------------------------------------------------------------
extern "C" __global__ void rank_pack_keys(const float* __restrict__ f, int n,
                                          unsigned* __restrict__ keys,
                                          unsigned* __restrict__ vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned u = __float_as_uint(f[i]);
  // float compare (and torch's sort) treats -0.0 == +0.0; the bit trick
  // would order them — canonicalize so they tie (index-order break).
  if ((u & 0x7FFFFFFFu) == 0u) u = 0u;
  keys[i] = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  vals[i] = (unsigned)i;
}

extern "C" __global__ void rank_scatter(const unsigned* __restrict__ vals,
                                        int n, float* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  out[vals[k]] = (float)k / (float)(n - 1) - 0.5f;
}

// ---------------------------------------------------------------------------
// Standalone batched policy forward (numerics target + serving op):
// logits[b][ACT] for X[b][OBS], unperturbed theta.  One workgroup per
// 64-row batch tile; same MFMA path as the rollout kernel.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
mlp_policy_forward(const float* __restrict__ theta,
                   const float* __restrict__ X, int batch,
                   float* __restrict__ logits) {
  __shared__ PolicyLds pol;
  __shared__ alignas(16) __hip_bfloat16 xb[ENVS][S1];
  __shared__ alignas(16) __hip_bfloat16 zero16[8];
  __shared__ alignas(16) __hip_bfloat16 h1[ENVS][S2];
  __shared__ alignas(16) __hip_bfloat16 h2[ENVS][S2];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int row0 = blockIdx.x * ENVS;

  for (int j = tid; j < NPARAMS; j += blockDim.x) store_param(&pol, j, theta[j]);
  for (int idx = tid; idx < HID * (S1 - OBS); idx += blockDim.x)
    pol.w1[idx / (S1 - OBS)][OBS + idx % (S1 - OBS)] =
        __float2bfloat16(0.f);
  for (int idx = tid; idx < ENVS * S1; idx += blockDim.x) {
    int e = idx / S1, d = idx % S1;
    float v = (d < OBS && row0 + e < batch) ? X[(row0 + e) * OBS + d] : 0.f;
    xb[e][d] = __float2bfloat16(v);
  }
  if (tid < 8) zero16[tid] = __float2bfloat16(0.f);
  __syncthreads();
  mfma_strip_tanh<KPAD, S1, S1, S2, true>(&pol.w1[0][0], &xb[0][0], pol.b1,
                                          &h1[0][0], wave, lane, zero16);
  __syncthreads();
  mfma_strip_tanh<HID, S2, S2, S2>(&pol.w2[0][0], &h1[0][0], pol.b2,
                                   &h2[0][0], wave, lane);
  __syncthreads();
  if (tid < ENVS && row0 + tid < batch) {
#pragma unroll
    for (int a = 0; a < ACT; ++a) {
      float l = pol.b3[a];
      for (int h = 0; h < HID; ++h)
        l += __bfloat162float(pol.w3[a][h]) *
             __bfloat162float(h2[tid][h]);
      logits[(row0 + tid) * ACT + a] = l;
    }
  }
}

// ---------------------------------------------------------------------------
// Raw MFMA refcheck kernel: C[64][64] = tanh-free A[64][64] x B[64][64]
// through the exact strip path used above (bias=0, output de-transposed
// host-side).  Lets the GPU test verify the fragment-layout assumptions
// with random asymmetric inputs (guide ERRATA #3: symmetric inputs can
// hide a transposed C-write).
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
mfma_gemm64_probe(const float* __restrict__ A64,
                  const float* __restrict__ B64,
                  float* __restrict__ C64T) {
  __shared__ alignas(16) __hip_bfloat16 a[HID][S2];
  __shared__ alignas(16) __hip_bfloat16 b[HID][S2];   // stored [col][k]
  __shared__ alignas(16) __hip_bfloat16 c[HID][S2];   // written [col][row]
  __shared__ alignas(16) float zero_bias[HID];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < HID * HID; idx += blockDim.x) {
    int r = idx >> 6, k = idx & 63;
    a[r][k] = __float2bfloat16(A64[r * HID + k]);
    // B stored transposed: b[col][k] = B[k][col]
    b[r][k] = __float2bfloat16(B64[k * HID + r]);
  }
  if (tid < HID) zero_bias[tid] = 0.f;
  __syncthreads();
  // tanh is applied by the strip helper; host compares against
  // tanh(A@B) to keep one code path.
  mfma_strip_tanh<HID, S2, S2, S2>(&a[0][0], &b[0][0], zero_bias, &c[0][0],
                                   tid >> 6, tid & 63);
  __syncthreads();
  for (int idx = tid; idx < HID * HID; idx += blockDim.x) {
    int col = idx >> 6, row = idx & 63;
    C64T[col * HID + row] = __bfloat162float(c[col][row]);
  }
}

// ---------------------------------------------------------------------------
// Logits-reduce probe: one wave takes per-lane partials p0[4][64] and
// p1[4][64] (4 column tiles x 64 lanes) through both forms of the
// cross-kgrp reduce and returns the lpart row each one writes, [ENVS][2].
// The rollout outputs see the logits only through l1 > l0; this compares
// the raw bits of the swap form (what the step loop runs) with the shfl
// tree it replaced.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(64)
logits_reduce_probe(const float* __restrict__ p0,  // [4][64]
                    const float* __restrict__ p1,  // [4][64]
                    float* __restrict__ out_shfl,  // [ENVS][2]
                    float* __restrict__ out_swap)  // [ENVS][2]
{
  __shared__ float lrow[2][ENVS][2];
  const int lane = threadIdx.x;
  float a[4], b[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    a[ct] = p0[ct * 64 + lane];
    b[ct] = p1[ct * 64 + lane];
  }
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
    logits_reduce_shfl(a[ct], b[ct], lrow[0], ct, lane);
#pragma unroll
  for (int cp = 0; cp < 4; cp += 2)
    logits_reduce_swap(a[cp], b[cp], a[cp + 1], b[cp + 1], lrow[1], cp, lane);
  __syncthreads();
#pragma unroll
  for (int a01 = 0; a01 < 2; ++a01) {
    out_shfl[lane * 2 + a01] = lrow[0][lane][a01];
    out_swap[lane * 2 + a01] = lrow[1][lane][a01];
  }
}

#endif  // ES_KERNELS_SHARED_ONLY
