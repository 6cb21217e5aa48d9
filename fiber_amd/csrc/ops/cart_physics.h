// CartPole's physics for the rollout kernels that step it (gfx950):
// cartpole_kernels.hip (MLP policy) and lstm_cartpole_kernels.hip (LSTM
// policy) include this one text, so a check of either covers the arithmetic
// of both.  fiber_amd/es/cartpole_oracle.py reads it operation by operation.
//
// Every fma and every separately rounded product is spelled out, so the
// compiler has no freedom in contraction.  Divisions are true IEEE divisions
// (__fdiv_rn), one per step; the divisions by mc + mp are products with a
// reciprocal formed once per launch.
#pragma once

#include <hip/hip_runtime.h>

#define CART_STATS 9  // sum[4], sumsq[4], count

// sin / cos as fixed Horner polynomials, odd through th^7 and even through
// th^8.  A live environment has |th| <= th_thr <= 0.5 (validated on the
// host), where the truncation error is under 6e-9 / 3e-10: no range
// reduction, and every operation can be bounded.
#define CART_S3 (-1.0f / 6.0f)
#define CART_S5 (1.0f / 120.0f)
#define CART_S7 (-1.0f / 5040.0f)
#define CART_C2 (-1.0f / 2.0f)
#define CART_C4 (1.0f / 24.0f)
#define CART_C6 (-1.0f / 720.0f)
#define CART_C8 (1.0f / 40320.0f)
#define CART_43 (4.0f / 3.0f)

// cart[8] = gravity, masscart, masspole, length (half the pole), force_mag,
// tau, x_threshold, theta_threshold; and what depends on them alone.
struct CartConst {
  float g, l, force, tau, x_thr, th_thr;
  float inv_total;  // 1 / (mc + mp)
  float pml;        // mp * l
  float mpt;        // mp / (mc + mp)
  float pmlt;       // mp * l / (mc + mp)
};

__device__ inline CartConst cart_consts(const float* __restrict__ cart) {
  CartConst k;
  k.g = cart[0];
  const float mc = cart[1], mp = cart[2];
  k.l = cart[3];
  k.force = cart[4];
  k.tau = cart[5];
  k.x_thr = cart[6];
  k.th_thr = cart[7];
  k.inv_total = __fdiv_rn(1.0f, mc + mp);
  k.pml = mp * k.l;
  k.mpt = mp * k.inv_total;
  k.pmlt = k.pml * k.inv_total;
  return k;
}

// One explicit-Euler step of Gym's CartPole-v1, in place.  Returns done,
// judged on the new state.
__device__ inline bool cart_physics(const CartConst& k, bool a, float& x,
                                    float& xd, float& th, float& thd) {
  const float t2 = th * th;
  const float sp = fmaf(t2, fmaf(t2, CART_S7, CART_S5), CART_S3);
  const float sn = fmaf(th, t2 * sp, th);
  const float cs = fmaf(
      t2, fmaf(t2, fmaf(t2, fmaf(t2, CART_C8, CART_C6), CART_C4), CART_C2),
      1.0f);
  const float force = a ? k.force : -k.force;
  const float temp = fmaf(k.pml * (thd * thd), sn, force) * k.inv_total;
  const float num = fmaf(-cs, temp, k.g * sn);
  const float den = k.l * fmaf(-k.mpt, cs * cs, CART_43);
  const float th_acc = __fdiv_rn(num, den);
  const float x_acc = fmaf(-(k.pmlt * th_acc), cs, temp);
  x = fmaf(k.tau, xd, x);
  xd = fmaf(k.tau, x_acc, xd);
  th = fmaf(k.tau, thd, th);
  thd = fmaf(k.tau, th_acc, thd);
  return fabsf(x) > k.x_thr || fabsf(th) > k.th_thr;
}
