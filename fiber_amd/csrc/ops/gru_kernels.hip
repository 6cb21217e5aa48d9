// GRU recurrent policy for the ES engine (gfx950): a gated cell 4 -> 64 -> 2
// with torch.nn.GRUCell's convention, rolled out for the whole horizon in
// one launch, one workgroup per population member.
//
//   r  = sigmoid(W_ir x + W_hr h + b_r)
//   z  = sigmoid(W_iz x + W_hz h + b_z)
//   n  = tanh   (W_in x + b_in + r * (W_hn h + b_hn))
//   h' = (1 - z) * n + z * h          (computed as n + z * (h - n))
//   logits = W_o h' + b_o             action = (l1 > l0), a tie is 0
//
//   es_rollout_gru   perturbed members, es_rollout_mlp's contract plus
//                    obs_mask and the optional final state / hidden state
//   gru_policy_step  one cell step for b rows: serving and numerics
//
// Both inline gru_cell, so a check of one covers the arithmetic of the other.
//
// Work split.  256 threads, 64 envs.  Wave w owns hidden rows 16w..16w+15 of
// all three gates for all four 16-env column tiles.  Its W_h A fragments (3
// gates x 2 K-tiles), the four bias quads and its W_o slice are
// loop-invariant and live in registers for the whole horizon.  Per column
// tile the B fragments of h (two K-tiles) and of x are read ONCE and feed
// all three gates; the three narrow W_i A fragments are read beside them,
// because the register budget has no room to keep them (GruRegs): 9 MFMAs
// on 6 fragment reads, where the feed-forward loop reads a fragment per
// MFMA.
//
// State in registers.  The C/D layout gives every lane rows drow..drow+3 of
// one env per tile, so the fp32 hidden state is 4 tiles x 4 values per lane
// and never leaves registers; the gate arithmetic is elementwise in that
// layout.  Only bf16(h'), the next step's B operand, goes to LDS: one packed
// 8-byte store per tile.  The carried state is NOT that rounded copy: bf16
// error would compound through z * h over the horizon.
//
// Two barriers per step.  The B operand of h is double-buffered: step t
// reads buffer t & 1 and writes the other, so nothing inside the MFMA phase
// and its epilogue needs a barrier.  The logits are formed in the epilogue
// from the fp32 h' (logits_reduce_swap into lpart); after a barrier comes
// the action / env step / reward / statistics / next-x phase, restated from
// rollout_steps with its fmaf forms and constants, then the second barrier.
//
// Rounding points mirror the MLP kernels: weights to bf16 when staged,
// biases fp32, the normalised clamped observation to bf16, the MFMA reads
// bf16(h), the logits read fp32 h'.
//
// The shared device code of es_kernels.hip (fragment helpers, fast_tanh, the
// logits reduce, Philox tags) is included without its kernels, as
// ga_kernels.hip and sm_kernels.hip do: a translation unit of its own cannot
// move the register allocation of es_rollout_mlp.

#define ES_KERNELS_SHARED_ONLY
#include "es_kernels.hip"

#define GATES 3  // r, z, n: torch's order

// flat theta layout
#define GOFF_WI 0                               // W_i[3][64][4]
#define GOFF_WH (GATES * HID * OBS)             // 768    W_h[3][64][64]
#define GOFF_B (GOFF_WH + GATES * HID * HID)    // 13056  b_r b_z b_in b_hn
#define GOFF_WO (GOFF_B + 4 * HID)              // 13312  W_o[2][64]
#define GOFF_BO (GOFF_WO + ACT * HID)           // 13440  b_o[2]
#define GRU_NPARAMS (GOFF_BO + ACT)             // 13442

#define GRU_WAVES 4  // waves per SIMD: 128 VGPRs; LDS allows 4 blocks per CU

#define LOG2E 0x1.715476p+0f

// sigmoid on the transcendental unit, next to fast_tanh:
// 1 / (1 + e^-a) = rcp(1 + exp2(-a * log2e)).  exp2 overflow gives inf and
// rcp(inf) = 0; underflow gives rcp(1) = 1.
__device__ inline float fast_sigmoid(float a) {
  const float e = __builtin_amdgcn_exp2f(a * -LOG2E);
  return __builtin_amdgcn_rcpf(1.0f + e);
}

struct GruLds {
  // W_h is only staged here until gru_load_regs has pulled its A fragments
  // into registers; the two B-operand buffers of h then live in the same
  // bytes, see hbuf().  27,648 B, of which the buffers use 18,432.
  alignas(16) __hip_bfloat16 wh[GATES][HID][S2];
  alignas(16) __hip_bfloat16 wi[GATES][HID][S1];
  alignas(16) float bias[4][HID];  // b_r, b_z, b_in, b_hn: read as quads
  alignas(16) __hip_bfloat16 wo[ACT][HID];
  float bo[ACT];
  alignas(16) __hip_bfloat16 xb[ENVS][S1];
  alignas(16) __hip_bfloat16 zero16[8];  // narrow kgrp>0 fragments
  float S[2][ENVS][OBS];     // env state (double-buffered)
  float lpart[4][ENVS][2];   // per-wave logits partials
  float ostat[2 * OBS + 1];

  // B operand of h for step parity k, [ENVS][S2].  Shares wh: nothing reads
  // W_h from LDS after gru_load_regs, every caller barriers between that
  // load and its first hbuf write, and the step loop only touches hbuf.
  // Do not read wh past that barrier.
  __device__ __hip_bfloat16* hbuf(int k) {
    return &wh[0][0][0] + k * (ENVS * S2);
  }
};
static_assert(2 * ENVS * S2 <= GATES * HID * S2,
              "both h buffers fit in the W_h staging tile");

__device__ inline void gru_store_param(GruLds* p, int j, float v) {
  if (j < GOFF_WH) {
    p->wi[j >> 8][(j >> 2) & 63][j & 3] = __float2bfloat16(v);
  } else if (j < GOFF_B) {
    const int jj = j - GOFF_WH;
    p->wh[jj >> 12][(jj >> 6) & 63][jj & 63] = __float2bfloat16(v);
  } else if (j < GOFF_WO) {
    (&p->bias[0][0])[j - GOFF_B] = v;
  } else if (j < GOFF_BO) {
    (&p->wo[0][0])[j - GOFF_WO] = __float2bfloat16(v);
  } else if (j < GRU_NPARAMS) {
    p->bo[j - GOFF_BO] = v;
  }
}

// The K-padding of W_i and xb (columns 4..7: A-side and B-side zeros) and
// the shared zero fragment.
__device__ inline void gru_init_pads(GruLds& L, int tid) {
  for (int idx = tid; idx < GATES * HID * (S1 - OBS); idx += blockDim.x)
    (&L.wi[0][0][0])[(idx / (S1 - OBS)) * S1 + OBS + idx % (S1 - OBS)] =
        __float2bfloat16(0.f);
  for (int idx = tid; idx < ENVS * (S1 - OBS); idx += blockDim.x)
    L.xb[idx / (S1 - OBS)][OBS + idx % (S1 - OBS)] = __float2bfloat16(0.f);
  if (tid < 8) L.zero16[tid] = __float2bfloat16(0.f);
}

// One lane's loop-invariant operands: 24 VGPRs of W_h A fragments, 16 of
// biases, 4 of W_o (kept as the bf16 pairs they are; widening is a shift and
// a mask per use, and as 8 floats they cost the last VGPRs under 128).  The
// narrow W_i fragments are not among them: with their 12 VGPRs resident the
// rollout kernel needs 142 and spills at the 128 that 4 waves/SIMD allow, so
// gru_cell reads them from LDS per column tile (three 16-byte reads beside
// the three of the B side; profiles/gru.md).
struct GruRegs {
  bf16x8 ah[GATES][HID / 32];
  f32x4 bq[4];
  uint32_t wop[4];  // rows drow..drow+3: bf16 (action 0 | action 1 << 16)
};

__device__ __forceinline__ void gru_load_regs(GruLds& L, int wave, int lane,
                                              GruRegs& R) {
#pragma unroll
  for (int g = 0; g < GATES; ++g)
    strip_load_a<HID, S2>(&L.wh[g][0][0], nullptr, wave, lane, R.ah[g]);
#pragma unroll
  for (int b = 0; b < 4; ++b) R.bq[b] = strip_load_bias(L.bias[b], wave, lane);
  const int drow = wave * 16 + (lane >> 4) * 4;
#pragma unroll
  for (int ri = 0; ri < 4; ++ri) {
    R.wop[ri] =
        (__float_as_uint(__bfloat162float(L.wo[0][drow + ri])) >> 16) |
        (__float_as_uint(__bfloat162float(L.wo[1][drow + ri])) & 0xffff0000u);
  }
}

// One cell step of this wave's 16 hidden rows for all 64 envs: reads x from
// xb and bf16(h) from hcur, updates the fp32 state h[tile] in place, writes
// bf16(h') to hnext[env][row] and the wave's logits partials to lpart[wave].
// No barrier inside; the caller separates hcur / hnext / lpart users.
__device__ __forceinline__ void gru_cell(
    const GruRegs& R, const __hip_bfloat16 (*wi)[HID][S1],
    const __hip_bfloat16* __restrict__ xb, const __hip_bfloat16* zero16,
    const __hip_bfloat16* __restrict__ hcur,
    __hip_bfloat16* __restrict__ hnext, f32x4 (&h)[4],
    float (*lpart)[ENVS][2], int wave, int lane) {
  const int drow = wave * 16 + (lane >> 4) * 4;
#pragma unroll
  for (int cp = 0; cp < 4; cp += 2) {
    float p0[2], p1[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int ct = cp + c;
      const int bcol = ct * 16 + (lane & 15);
      // three fragment reads feed nine MFMAs
      const bf16x8 bx =
          *strip_frag_ptr<S1, true>(xb, zero16, bcol, 0, lane >> 4);
      const bf16x8 bh0 =
          *strip_frag_ptr<S2, false>(hcur, nullptr, bcol, 0, lane >> 4);
      const bf16x8 bh1 =
          *strip_frag_ptr<S2, false>(hcur, nullptr, bcol, 1, lane >> 4);
      bf16x8 ai[GATES][1];
#pragma unroll
      for (int g = 0; g < GATES; ++g)
        strip_load_a<KPAD, S1, true>(&wi[g][0][0], zero16, wave, lane, ai[g]);
      // The fp32 bias quads have the C/D layout (rows drow..drow+3), so
      // each accumulator starts from its bias: no add in the epilogue.
      // r and z: x part and h part summed in one accumulator
      f32x4 ar = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ai[0][0], bx,
                                                         R.bq[0], 0, 0, 0);
      f32x4 az = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ai[1][0], bx,
                                                         R.bq[1], 0, 0, 0);
      // n: the two parts stay apart for the r * (...) product
      const f32x4 anx = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          ai[2][0], bx, R.bq[2], 0, 0, 0);
      f32x4 anh = __builtin_amdgcn_mfma_f32_16x16x32_bf16(R.ah[2][0], bh0,
                                                          R.bq[3], 0, 0, 0);
      ar = __builtin_amdgcn_mfma_f32_16x16x32_bf16(R.ah[0][0], bh0, ar, 0, 0,
                                                   0);
      az = __builtin_amdgcn_mfma_f32_16x16x32_bf16(R.ah[1][0], bh0, az, 0, 0,
                                                   0);
      anh = __builtin_amdgcn_mfma_f32_16x16x32_bf16(R.ah[2][1], bh1, anh, 0,
                                                    0, 0);
      ar = __builtin_amdgcn_mfma_f32_16x16x32_bf16(R.ah[0][1], bh1, ar, 0, 0,
                                                   0);
      az = __builtin_amdgcn_mfma_f32_16x16x32_bf16(R.ah[1][1], bh1, az, 0, 0,
                                                   0);
      union {
        __hip_bfloat16 b[4];
        unsigned long long u;
      } pk;
      float q0 = 0.f, q1 = 0.f;
#pragma unroll
      for (int ri = 0; ri < 4; ++ri) {
        const float r = fast_sigmoid(ar[ri]);
        const float z = fast_sigmoid(az[ri]);
        // one fma, spelled out so that both kernels round it alike
        const float n = fast_tanh(fmaf(r, anh[ri], anx[ri]));
        // (1 - z) * n + z * h
        const float hn = fmaf(z, h[ct][ri] - n, n);
        h[ct][ri] = hn;
        pk.b[ri] = __float2bfloat16(hn);
        q0 = fmaf(__uint_as_float(R.wop[ri] << 16), hn, q0);
        q1 = fmaf(__uint_as_float(R.wop[ri] & 0xffff0000u), hn, q1);
      }
      *reinterpret_cast<unsigned long long*>(&hnext[bcol * S2 + drow]) = pk.u;
      p0[c] = q0;
      p1[c] = q1;
    }
    logits_reduce_swap(p0[0], p1[0], p0[1], p1[1], lpart[wave], cp, lane);
  }
}

extern "C" __global__ void __launch_bounds__(256, GRU_WAVES)
es_rollout_gru(const float* __restrict__ theta, float sigma, uint32_t seed,
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
               float* __restrict__ final_hidden)   // [pop_shard][64][64]/null
{
  __shared__ GruLds L;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int member = member_offset + blockIdx.x;
  const uint32_t pair = (uint32_t)(member >> 1);
  const float sgn = (member & 1) ? -sigma : sigma;

  // ---- fill the perturbed policy into LDS ------------------------------
  for (int jb = tid; jb * 4 < GRU_NPARAMS; jb += blockDim.x) {
    float z[4];
    fam_normal4(seed, iter, pair, (uint32_t)jb, FAM_TAG_NOISE, 0u, z);
    const int j0 = jb * 4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u;
      if (j < GRU_NPARAMS) gru_store_param(&L, j, fmaf(sgn, z[u], theta[j]));
    }
  }
  gru_init_pads(L, tid);
  // env init state: member-independent, common random numbers
  if (tid < ENVS) {
    float z[4];
    fam_normal4(seed, iter, (uint32_t)tid, 0u, FAM_TAG_ENV, 0u, z);
#pragma unroll
    for (int d = 0; d < OBS; ++d) L.S[0][tid][d] = 0.3f * z[d];
  }
  if (tid < 2 * OBS + 1) L.ostat[tid] = 0.f;
  __syncthreads();

  GruRegs R;
  gru_load_regs(L, wave, lane, R);
  // every wave's W_h fragment reads are done before any hbuf write
  __syncthreads();
  // h = 0 at the start of the episode: the registers and buffer 0
  f32x4 h[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) h[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int idx = tid; idx < ENVS * (HID / 4); idx += blockDim.x)
    *reinterpret_cast<unsigned long long*>(
        &L.hbuf(0)[(idx >> 4) * S2 + (idx & 15) * 4]) = 0ull;

  // ---- the D2 phase's per-thread state, as in rollout_steps ------------
  const int env = tid & 63;
  // dd = wave, made visibly wave-uniform so that the eight constants below
  // sit in SGPRs: as VGPRs they push the step loop past its 128
  const int dd = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0..3
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
  if (horizon > 0) {
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
    // ---- gates, h', logits partials (MFMA, one phase) ------------------
    gru_cell(R, L.wi, &L.xb[0][0], L.zero16, L.hbuf(cur), L.hbuf(cur ^ 1), h,
             L.lpart, wave, lane);
    __syncthreads();
    // ---- action, env step, reward, stats, next xb ----------------------
    {
      const float l0 = L.bo[0] + L.lpart[0][env][0] + L.lpart[1][env][0] +
                       L.lpart[2][env][0] + L.lpart[3][env][0];
      const float l1 = L.bo[1] + L.lpart[0][env][1] + L.lpart[1][env][1] +
                       L.lpart[2][env][1] + L.lpart[3][env][1];
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

  // Everything below is addressed from a copy of tid that the compiler
  // cannot see through: computed from tid itself, the output addresses are
  // hoisted above the step loop, stay live through it and spill (3 VGPRs of
  // scratch at the 128-VGPR budget).
  int etid = tid;
  asm volatile("" : "+v"(etid));
  const int eenv = etid & 63, edd = etid >> 6, elane = etid & 63;

  // ---- optional outputs: never touch what fitness / stats read ---------
  if (final_state != nullptr)
    final_state[((size_t)blockIdx.x * ENVS + eenv) * OBS + edd] =
        L.S[horizon & 1][eenv][edd];
  if (final_hidden != nullptr) {
    const int drow = edd * 16 + (elane >> 4) * 4;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
      *reinterpret_cast<f32x4*>(
          &final_hidden[((size_t)blockIdx.x * ENVS + ct * 16 + (elane & 15)) *
                            HID + drow]) = h[ct];
  }

  // ---- epilogue: fitness + obs-stat reductions, as es_rollout_mlp ------
  L.lpart[edd][eenv][0] = raccp;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    psum += __shfl_down(psum, off, 64);
    psq += __shfl_down(psq, off, 64);
  }
  if (elane == 0) {
    L.ostat[edd] = psum;
    L.ostat[OBS + edd] = psq;
  }
  __syncthreads();
  if (edd == 0) {
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
// normalised) and H[b][64]: logits[b][2], Hnew[b][64].  Tail rows past b
// compute on zeros and store nothing.
extern "C" __global__ void __launch_bounds__(256, GRU_WAVES)
gru_policy_step(const float* __restrict__ theta, const float* __restrict__ X,
                const float* __restrict__ H, int batch,
                float* __restrict__ logits, float* __restrict__ Hnew) {
  __shared__ GruLds L;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const size_t row0 = (size_t)blockIdx.x * ENVS;

  for (int j = tid; j < GRU_NPARAMS; j += blockDim.x)
    gru_store_param(&L, j, theta[j]);
  gru_init_pads(L, tid);
  {
    const int e = tid & 63, d = tid >> 6;
    const size_t row = row0 + e;
    L.xb[e][d] =
        __float2bfloat16(row < (size_t)batch ? X[row * OBS + d] : 0.f);
  }
  __syncthreads();

  GruRegs R;
  gru_load_regs(L, wave, lane, R);
  __syncthreads();  // W_h fragment reads done: hbuf may be written

  // this lane's fp32 h in the C/D layout, and bf16(h) as the B operand
  const int drow = wave * 16 + (lane >> 4) * 4;
  f32x4 h[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int e = ct * 16 + (lane & 15);
    const size_t row = row0 + e;
    h[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (row < (size_t)batch)
      h[ct] = *reinterpret_cast<const f32x4*>(&H[row * HID + drow]);
    union {
      __hip_bfloat16 b[4];
      unsigned long long u;
    } pk;
#pragma unroll
    for (int ri = 0; ri < 4; ++ri) pk.b[ri] = __float2bfloat16(h[ct][ri]);
    *reinterpret_cast<unsigned long long*>(&L.hbuf(0)[e * S2 + drow]) = pk.u;
  }
  __syncthreads();

  gru_cell(R, L.wi, &L.xb[0][0], L.zero16, L.hbuf(0), L.hbuf(1), h, L.lpart,
           wave, lane);
  __syncthreads();

#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const size_t row = row0 + ct * 16 + (lane & 15);
    if (row < (size_t)batch)
      *reinterpret_cast<f32x4*>(&Hnew[row * HID + drow]) = h[ct];
  }
  if (tid < ENVS * ACT) {
    const int e = tid >> 1, a = tid & 1;
    const size_t row = row0 + e;
    if (row < (size_t)batch)
      logits[row * ACT + a] = L.bo[a] + L.lpart[0][e][a] + L.lpart[1][e][a] +
                              L.lpart[2][e][a] + L.lpart[3][e][a];
  }
}
