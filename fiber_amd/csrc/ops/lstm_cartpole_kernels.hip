// The LSTM policy on CartPole (gfx950): pole balancing where the policy may
// be shown the positions only and has to recover the velocities from memory.
//
//   es_rollout_lstm_cartpole  one workgroup of 512 threads per member, 64
//                             environments, the whole horizon in one launch
//
// The policy, its theta layout, its Philox draws and its rounding points are
// es_rollout_lstm's: lstm_load and lstm_cell are that file's text, included
// below without its kernels.  The environment is es_rollout_mlp_cartpole's:
// cart_consts and cart_physics are cart_physics.h, the start states are
// 0.05 z of the FAM_TAG_ENV draw, an episode ends on the new state, the
// terminating step counts, and the fitness is the mean episode length (an
// integer sum, then one conversion).  es_grad(nparams = LSTM_NPARAMS),
// centered_rank and cartpole_stat_reduce serve it unchanged.
//
// Neither kernel's step loop carries over.  The MLP kernel packs the live
// environments into the leading column tiles every step, which it can do
// because its policy keeps nothing per environment.  Here the fp32 cell
// state of an environment sits in the C/D registers of one MFMA column for
// the whole horizon, so:
//
// * Environments never move.  Wave (strip = w & 3, half = w >> 2) owns 16
//   hidden rows of all four gates for column tiles 2 half and 2 half + 1, as
//   in es_rollout_lstm, and c stays in its 8 VGPRs.
// * The live mask is wave-uniform.  In the env phase lane e of EVERY wave
//   reads the state of environment e as one 16-byte LDS vector and steps it.
//   The eight waves run the same instructions on the same inputs, so
//   live = __ballot(still alive) is the same 64-bit mask in all of them
//   without an exchange (cartpole_kernels.hip's argument), it is carried in
//   scalar registers, `if (live == 0) break;` is uniform across the block and
//   the barrier counts stay matched.
// * Dead tiles cost nothing.  Column tile j is live iff bits 16 j .. 16 j + 15
//   of the mask are not all zero, a scalar test: lstm_cell<true> skips the 12
//   MFMAs, the 40 transcendentals and the bf16(h') store of a dead tile, and
//   a wave whose two tiles are dead skips the phase and only meets the two
//   barriers.  A dead environment inside a live tile keeps computing on
//   stale finite inputs (|h| <= 1, |c| grows by at most 1 per step, its xb
//   row keeps its last value); a column of D depends only on its column of
//   B, so it cannot touch a live one, and nothing of it is read back.
// * State in LDS, transients in registers.  The four state floats are
//   L.S[parity][env], double-buffered like es_rollout_lstm's.  Only waves
//   d < 4 write: dim d of the new state (a dead environment's old value, so
//   that it stays frozen bit for bit in both buffers), the statistics
//   partials of dim d and xb[env][d].  The episode length is not carried:
//   wave 0 stores t + 1 to LDS at the terminating step, and an environment
//   still alive after the loop took every step that ran.  CartConst is
//   uniform.  The loop carries c (8), the policy (52) and psum / psq: one
//   VGPR fewer than es_rollout_lstm.
//
// Statistics cover the states presented to the policy, as in
// es_rollout_mlp_cartpole: the start state if any step runs, and every new
// state of an environment that is still alive and has a step left.

#define LSTM_KERNELS_SHARED_ONLY
#include "lstm_kernels.hip"

#include "cart_physics.h"

// dim d of a state held in four registers, d wave-uniform
__device__ __forceinline__ float lc_dim(int d, float s0, float s1, float s2,
                                        float s3) {
  return d == 0 ? s0 : d == 1 ? s1 : d == 2 ? s2 : s3;
}

extern "C" __global__ void __launch_bounds__(LSTM_THREADS, LSTM_WAVES)
es_rollout_lstm_cartpole(const float* __restrict__ theta, float sigma,
                         uint32_t seed, uint32_t iter, int horizon,
                         int member_offset,
                         const float* __restrict__ obs_mu,
                         const float* __restrict__ obs_nu,
                         const float* __restrict__ cart,     // [8]
                         int obs_mask,                       // bit d: visible
                         float* __restrict__ fitness,        // [pop]
                         float* __restrict__ stat_part,      // [pop][9]
                         int* __restrict__ lengths,          // [pop][64] / 0
                         float* __restrict__ final_state,    // [pop][64][4]/0
                         float* __restrict__ final_hidden,   // [pop][64][64]/0
                         float* __restrict__ final_cell)     // [pop][64][64]/0
{
  __shared__ LstmLds L;
  __shared__ int ended_at[ENVS];  // t + 1 of the terminating step
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int member = member_offset + blockIdx.x;
  const uint32_t pair = (uint32_t)(member >> 1);
  const float sgn = (member & 1) ? -sigma : sigma;

  // env init state: member-independent, common random numbers
  if (tid < ENVS) {
    float z[4];
    fam_normal4(seed, iter, (uint32_t)tid, 0u, FAM_TAG_ENV, 0u, z);
    *reinterpret_cast<f32x4*>(&L.S[0][tid][0]) =
        (f32x4){0.05f * z[0], 0.05f * z[1], 0.05f * z[2], 0.05f * z[3]};
  }
  // h = c = 0 at the start of the episode: buffer 0 and the registers.  hfin
  // stays zero unless the last step runs.
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

  // ---- the env phase's uniform state ------------------------------------
  // Waves 0..3 write dim dd = wave; waves 4..7 load the constants of
  // dd = wave - 4 and never use them.
  const bool env_wave = wave < OBS;
  const int dd = wave & (OBS - 1);
  const int half = wave >> 2;
  const float mu_d = obs_mu[dd];
  const float rstd_d = rsqrtf(obs_nu[dd] + 1e-4f);
  const bool visible = (obs_mask >> dd) & 1;
  const CartConst k = cart_consts(cart);
  float psum = 0.f, psq = 0.f;
  unsigned long long live = ~0ull;  // the same in every wave: SGPRs

  // prologue for t = 0: stats + normalised obs from the init state
  if (horizon > 0 && env_wave) {
    const float s = L.S[0][lane][dd];
    psum += s;
    psq = fmaf(s, s, psq);
    const float x = (s - mu_d) * rstd_d;
    L.xb[lane][dd] =
        __float2bfloat16(visible ? fminf(5.f, fmaxf(-5.f, x)) : 0.f);
  }

  int t = 0;
  for (; t < horizon; ++t) {
    if (live == 0) break;  // uniform across the block
    const int cur = t & 1;
    // this wave's two column tiles, 16 mask bits each
    const uint32_t mine = (uint32_t)(live >> (32 * half));
    const int tiles = ((mine & 0xffffu) ? 1 : 0) | ((mine >> 16) ? 2 : 0);
    __syncthreads();
    // ---- gates, c', h', logits partials of the live tiles ---------------
    if (tiles != 0)
      lstm_cell<true>(R, L.wi, &L.xb[0][0], L.zero16, &L.hb[cur][0][0],
                      &L.hb[cur ^ 1][0][0], c,
                      t == horizon - 1 ? &L.hfin[0][0] : nullptr,
                      L.lpart[wave & 3], wave & 3, half, lane, tiles);
    __syncthreads();
    // ---- action and physics of environment `lane`, in every wave --------
    // A dead environment's logits and state are stale but finite; what is
    // computed from them is dropped.
    const f32x4 s = *reinterpret_cast<const f32x4*>(&L.S[cur][lane][0]);
    const float l0 = L.small[LS_BO] + L.lpart[0][lane][0] +
                     L.lpart[1][lane][0] + L.lpart[2][lane][0] +
                     L.lpart[3][lane][0];
    const float l1 = L.small[LS_BO + 1] + L.lpart[0][lane][1] +
                     L.lpart[1][lane][1] + L.lpart[2][lane][1] +
                     L.lpart[3][lane][1];
    const bool alive = (live >> lane) & 1;
    float x = s[0], xd = s[1], th = s[2], thd = s[3];
    const bool done = cart_physics(k, l1 > l0, x, xd, th, thd);
    const bool still = alive && !done;
    if (env_wave) {
      const float snew = alive ? lc_dim(dd, x, xd, th, thd)
                               : lc_dim(dd, s[0], s[1], s[2], s[3]);
      L.S[cur ^ 1][lane][dd] = snew;  // frozen once the episode has ended
      if (still && t < horizon - 1) {
        psum += snew;
        psq = fmaf(snew, snew, psq);
        const float xn = (snew - mu_d) * rstd_d;
        L.xb[lane][dd] =
            __float2bfloat16(visible ? fminf(5.f, fmaxf(-5.f, xn)) : 0.f);
      }
    }
    if (wave == 0 && alive && done) ended_at[lane] = t + 1;
    live = __ballot(still);
  }
  __syncthreads();
  // t is now the number of steps that ran; the last state is in S[t & 1]

  // Everything below is addressed from a fresh opaque copy of tid (lstm_tid).
  const int etid = lstm_tid();
  const int elane = etid & 63, ewave = etid >> 6;

  // ---- optional outputs: never touch what fitness / stats read ----------
  if (final_state != nullptr && etid < LSTM_ENV_THREADS)
    final_state[((size_t)blockIdx.x * ENVS + elane) * OBS + ewave] =
        L.S[t & 1][elane][ewave];
  {
    const int drow = (ewave & 3) * 16 + (elane >> 4) * 4;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      // each lane reads back what it wrote itself; the rows of an
      // environment that has ended are zero
      const int e = ((ewave >> 2) * 2 + cc) * 16 + (elane & 15);
      const bool e_alive = (live >> e) & 1;
      const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
      const size_t at = ((size_t)blockIdx.x * ENVS + e) * HID + drow;
      if (final_hidden != nullptr)
        *reinterpret_cast<f32x4*>(&final_hidden[at]) =
            e_alive ? *reinterpret_cast<const f32x4*>(&L.hfin[e][drow])
                    : zero;
      if (final_cell != nullptr)
        *reinterpret_cast<f32x4*>(&final_cell[at]) = e_alive ? c[cc] : zero;
    }
  }

  // ---- epilogue: a fixed shuffle tree per wave, no float atomics --------
  float* __restrict__ row = stat_part + (size_t)blockIdx.x * CART_STATS;
  if (ewave < OBS) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      psum += __shfl_down(psum, off, 64);
      psq += __shfl_down(psq, off, 64);
    }
    if (elane == 0) {
      row[ewave] = psum;
      row[OBS + ewave] = psq;
    }
  }
  if (ewave != 0) return;
  const int len = ((live >> elane) & 1) ? t : ended_at[elane];
  if (lengths != nullptr) lengths[(size_t)blockIdx.x * ENVS + elane] = len;
  int total = len;  // exact: an integer sum, then one conversion
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    total += __shfl_down(total, off, 64);
  if (elane == 0) {
    fitness[blockIdx.x] = (float)total / (float)ENVS;
    row[2 * OBS] = (float)total;
  }
}
