"""Float64 oracle of LM-MA-ES as fiber_amd/es/lmmaes.py runs it, and of the
low-rank perturbation kernels under it (CPU only, numpy).

The transform ``d = T z`` is written here in the paper's *chain* form
(Loshchilov, Glasmachers, Beyer 2019, Algorithm 1)

    d <- (1 - c_d[j]) d + c_d[j] m_j (m_j . d),   j = 1 .. J

while the engine and the kernels use the closed form ``T = scale * I +
dirs^t mix dirs``: comparing the two checks the closed form.

``lowrank_params`` is the kernels' arithmetic for any ``(dirs, mix, scale)``
in float64, with a bound on ``|kernel's fp32 value - this value|`` per
parameter, derived like cartpole_oracle.py's: the triangle inequality
through every operation and ``U`` times its result for each fp32 rounding
on the path, the draws known to ``Z_REL``.  The depths are those of
``lowrank_fill`` (lowrank_kernels.hip) as written:

  p[k]  20 fmas in the thread (5 slots x 4), 3 halving adds and 3
        butterfly adds in the wave, 3 adds over the 4 waves: 29 roundings,
        each of a partial sum that never exceeds A[k] = sum_j |dirs[k][j]
        z[j]|
  b[k]  an fma chain over l <= k: k + 1 roundings of partial sums within
        sum_l |mix[k][l] p[l]|
  d[j]  scale * z[j] rounded (scale itself is the nearest fp32 of the
        caller's float), then J fmas
  out   theta[j] + sgn * d[j], one fma

What the functions return is that bound times ``SAFETY``, the constant of
rollout_oracle.py.  Nothing here is fitted to what a device returned.
"""

import math

import numpy as np

from . import update_oracle as UO
from .rollout_oracle import SAFETY, U, Z_REL

NPARAMS = 4610
P_DEPTH = 20 + 6 + 3


# ---- the algorithm ----------------------------------------------------------

def default_n_dirs(n=NPARAMS):
    """m = lambda_0 = 4 + floor(3 ln n): 29 at n = 4610."""
    return 4 + int(math.floor(3.0 * math.log(n)))


def paper_rates(n_dirs, n=NPARAMS):
    """``(c_sigma, c_d[m], c_c[m])`` at the paper's default population
    lambda_0 (not the run's)."""
    lam0 = default_n_dirs(n)
    i = np.arange(n_dirs, dtype=np.float64)
    return 2.0 * lam0 / n, 1.0 / (1.5 ** i * n), lam0 / (4.0 ** i * n)


def transform_chain(dirs, c_d, z):
    """``T z`` by the paper's chain, float64; ``dirs[J][n]``, ``c_d[J]``."""
    d = np.array(z, dtype=np.float64)
    for m, c in zip(np.asarray(dirs, dtype=np.float64),
                    np.asarray(c_d, dtype=np.float64)):
        d = (1.0 - c) * d + c * m * (m @ d)
    return d


def weights(lam):
    """``(w[lam], mu_w)``: w[i - 1] is the weight of the member at position
    i (1 is the best), ``max(0, ln(mu + 1/2) - ln i)`` normalised to sum 1;
    exactly mu = lam / 2 of them are positive."""
    mu = lam // 2
    i = np.arange(1, lam + 1, dtype=np.float64)
    w = np.maximum(0.0, math.log(mu + 0.5) - np.log(i))
    w /= w.sum()
    return w, 1.0 / float((w * w).sum())


def wpair_from_fitness(fitness):
    """``(wpair[lam / 2], bound)`` from fp32 fitness: the member of integer
    rank r (0 is the worst, ties in index order as ``ops.centered_rank``
    breaks them) sits at position lam - r.  The engine gathers the weights
    from an fp32 table (U of each) and subtracts once."""
    r = UO.ranks_exact(fitness)
    w, _ = weights(r.size)
    wm = w[r.size - 1 - r]
    wp = wm[0::2] - wm[1::2]
    return wp, U * (wm[0::2] + wm[1::2]) + U * np.abs(wp)


# ---- the kernels ------------------------------------------------------------

def lowrank_params(theta, sgn, z, dirs, mix, scale):
    """``(params[n], bound[n])`` of one member: ``theta + sgn * (scale * z
    + dirs^t (tril(mix) (dirs z)))``.  theta, z, dirs, mix are the fp32
    values the kernel reads (z numpy's float32 draw), ``sgn`` the fp32 +-
    sigma, ``scale`` the caller's float."""
    theta, z, dirs, mix = (np.asarray(a, dtype=np.float32).astype(np.float64)
                           for a in (theta, z, dirs, mix))
    J = dirs.shape[0]
    sgn = float(np.float32(sgn))
    s32 = float(np.float32(scale))
    mix = np.tril(mix).reshape(J, J)
    az = np.abs(z)
    A = np.abs(dirs) @ az
    p = dirs @ z
    p_err = (P_DEPTH * U + Z_REL) * A
    b = mix @ p
    b_err = np.abs(mix) @ p_err + (np.arange(J) + 1.0) * U * (
        np.abs(mix * p[None, :]).sum(axis=1))
    sz = s32 * z
    d = sz + dirs.T @ b
    mag = np.abs(sz) + np.abs(dirs).T @ np.abs(b)
    d_err = (np.abs(sz) * (Z_REL + U) + np.abs(dirs).T @ b_err
             + (J + 1.0) * U * mag)
    out = theta + sgn * d
    return out, SAFETY * (abs(sgn) * d_err + U * np.abs(out))


# ---- one engine update ------------------------------------------------------

def step_fp64(state, fitness, cfg, lm, iteration):
    """One ``LMMAESEngine.step()`` in float64 from the fp32 pre-step
    ``state`` (theta, sigma, p_sigma, dirs, t_step) and the device's own
    fp32 ``fitness``.  ``cfg`` is the ESConfig, ``lm`` the resolved
    LMMAESConfig.  Returns ``(new, tol)``: the new state and a bound per
    element on |device - new| (with SAFETY).

    The engine's sequence, one U per fp32 operation torch performs, a Python
    scalar entering one rounded to fp32 first (update_oracle.py's rules):
    g_z is ``es_grad`` (``grad_tol``); g_d = T g_z is formed in float64 on
    the device from the fp32 g_z and rounded once; ``theta.add_(g_d,
    alpha)`` rounds alpha, the product and the sum; p_sigma and every row of
    dirs are ``x.mul_(decay).add_(coef * g_z)`` with decay and coef fp32:
    their own rounding, the two products and the sum.  sigma is a Python
    float: the only error it inherits is p_sigma's, through the norm."""
    f64 = UO._f64
    n = NPARAMS
    theta, p_sig, dirs = f64(state["theta"]), f64(state["p_sigma"]), f64(
        state["dirs"])
    sigma, t = float(state["sigma"]), int(state["t_step"])
    lam = np.asarray(fitness).size
    c_d, c_c = np.asarray(lm.c_d, np.float64), np.asarray(lm.c_c, np.float64)
    J = min(t, dirs.shape[0])

    w, w_err = wpair_from_fitness(fitness)
    _, mu_w = weights(lam)
    g_z, abs_sum, spread = UO.grad_fp64(w, 0, lam // 2, cfg.seed, iteration,
                                        n, w_err=w_err)
    gz_tol = UO.grad_tol(abs_sum, lam // 2,
                         UO.grad_chunks(lam // 2, n)) + spread

    # g_d = T g_z: |T| <= a I + sum_j c_d[j] |m_j| |m_j|^t applied in chain
    g_d = transform_chain(dirs[:J], c_d[:J], g_z)
    gd_tol = gz_tol.copy()
    for m, c in zip(np.abs(dirs[:J]), c_d[:J]):
        gd_tol = (1.0 - c) * gd_tol + c * m * (m @ gd_tol)
    gd_tol = gd_tol + U * np.abs(g_d)

    alpha = float(lm.lr_mean) * sigma
    new_theta = theta + alpha * g_d
    theta_tol = (abs(alpha) * gd_tol + 2.0 * U * np.abs(alpha * g_d)
                 + U * np.abs(new_theta))

    def blend(x, decay, coef):
        """x.mul_(decay).add_(coef * g_z) and its bound."""
        new = decay * x + coef * g_z
        return new, (2.0 * U * np.abs(decay * x) + coef * gz_tol
                     + 2.0 * U * np.abs(coef * g_z) + U * np.abs(new))

    cs = float(lm.c_sigma)
    new_p, p_tol = blend(p_sig, 1.0 - cs, math.sqrt(mu_w * cs * (2.0 - cs)))
    new_dirs, dirs_tol = blend(dirs, (1.0 - c_c)[:, None],
                               np.sqrt(mu_w * c_c * (2.0 - c_c))[:, None])

    norm2 = float(new_p @ new_p)
    norm2_tol = float((2.0 * np.abs(new_p) * p_tol + p_tol * p_tol).sum())
    factor = math.exp(0.5 * cs * (norm2 / n - 1.0))
    new_sigma = min(max(sigma * factor, lm.sigma_min), lm.sigma_max)
    # the device sums the n squares in float64 (any order: n * 2^-53 of the
    # sum); exp, the products and the division are float64 on the host
    sigma_tol = new_sigma * (
        0.5 * cs / n * (norm2_tol + n * 2.0 ** -53 * norm2) + 8.0 * 2.0 ** -53)

    new = {"theta": new_theta, "p_sigma": new_p, "dirs": new_dirs,
           "sigma": new_sigma, "t_step": t + 1, "n_active": J}
    tol = {"theta": SAFETY * theta_tol, "p_sigma": SAFETY * p_tol,
           "dirs": SAFETY * dirs_tol, "sigma": SAFETY * sigma_tol}
    return new, tol
