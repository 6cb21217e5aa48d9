"""Float64 oracle of the step-size half of a separable-NES iteration (CPU
only, numpy only).

``update_oracle`` covers what turns fitness into a new ``theta``; this adds
what turns it into a new ``sigma``: the ``g_sig`` row of ``es_grad_sigma``
(fiber_amd/csrc/ops/snes_kernels.hip) and the sigma lines of
``SNESEngine.step`` (fiber_amd/es/snes.py).  It is written from those
sources on top of ``update_oracle``'s draws, chunk split and exact ranks.

The derivations are in profiles/snes.md; ``U`` is one fp32 rounding, ``ULP``
one ulp of a device function, as in ``rollout_oracle``.
"""

import numpy as np

from . import update_oracle as uo
from .rollout_oracle import U, ULP, Z_SIDE_ULPS


def sigma_grad_fp64(wsum, pair_begin, pair_end, seed, iteration, nparams,
                    jb=None, w_err=None):
    """``(g_sig, abs_sum)``: ``g_sig[j] = sum_k wsum[k] (z_k[j]^2 - 1)`` over
    the pairs ``pair_begin <= k < pair_end`` and ``abs_sum[j] = sum_k
    |wsum[k]| (z_k[j]^2 + 1)``, at ``param_index(nparams, jb)``.  ``wsum``
    is indexed by the pair number, like the kernel's; nothing outside the
    range is read.  With ``w_err`` (a bound on each weight's own error) a
    third array ``sum_k w_err[k] |z_k[j]^2 - 1|`` is returned."""
    w = np.asarray(wsum).astype(np.float64)
    n = uo.param_index(nparams, jb).size
    g = np.zeros(n)
    abs_sum = np.zeros(n)
    spread = np.zeros(n)
    for k in range(int(pair_begin), int(pair_end)):
        z = uo.noise_fp64(seed, iteration, k, nparams, jb)
        zz = z * z
        g += w[k] * (zz - 1.0)
        abs_sum += np.abs(w[k]) * (zz + 1.0)
        if w_err is not None:
            spread += w_err[k] * np.abs(zz - 1.0)
    if w_err is not None:
        return g, abs_sum, spread
    return g, abs_sum


def sigma_grad_tol(abs_sum, pairs, chunks):
    """Bound on |es_grad_sigma's g_sig - sigma_grad_fp64|, relative to
    ``abs_sum``: each draw is known to Z_SIDE_ULPS ulp, so z^2 to twice
    that; q = fma(z, z, -1) rounds once, at most U (z^2 + 1); acc = fma(w,
    q, acc) rounds once per accumulate over the at most ``per_chunk`` pairs
    of a chunk, and es_grad_reduce adds the ``chunks`` partials."""
    per_chunk = (pairs + chunks - 1) // chunks
    return (2.0 * Z_SIDE_ULPS * ULP + (1 + per_chunk + chunks) * U
            ) * np.asarray(abs_sum, dtype=np.float64)


def sigma_step_fp64(sigma, fitness, cfg, snes, seed, iteration, nparams):
    """The sigma lines of one ``SNESEngine.step()`` in float64, from the fp32
    pre-step ``sigma[nparams]`` and the device's own fp32 ``fitness`` of the
    whole population (exact ranks, as in ``step_fp64``).  ``snes`` carries
    the concrete ``lr_sigma``, ``sigma_min`` and ``sigma_max``
    (``SNESEngine.snes``).  ``cfg`` is the engine's ``ESConfig``, taken as
    ``step_fp64`` takes it; the sigma lines read only ``pop_per_gpu`` from
    it, which must be the size of ``fitness``.

    Returns ``(new_sigma, tol, clamp_flag)``: the new vector, a bound per
    element on |device - new_sigma|, and a mask of the coordinates whose
    unclamped reference lies within its tolerance of either rail: there the
    device may land on either side of the clamp, and the coordinate is not
    comparable.

    Tolerance, first order: the product p = g_sig * c with c = 0.5 *
    lr_sigma / pop carries g_sig's bound times c, U for c entering the
    tensor operation as fp32 and U for the product; exp(p) is allowed ULP
    relative to its result and moves by exp(p) * |dp|; the product with
    sigma rounds once more.  A coordinate clearly beyond a rail is the
    rail's fp32 value exactly."""
    if snes.lr_sigma is None or snes.sigma_min is None or (
            snes.sigma_max is None):
        raise ValueError("sigma_step_fp64 needs a resolved SNES config")
    fit = np.asarray(fitness, dtype=np.float32).reshape(-1)
    pop_total = fit.size
    if pop_total != int(cfg.pop_per_gpu):
        raise ValueError("fitness holds %d members, cfg.pop_per_gpu is %d"
                         % (pop_total, cfg.pop_per_gpu))
    pairs = pop_total // 2
    sig0 = np.asarray(sigma, dtype=np.float32).astype(np.float64).reshape(-1)
    assert sig0.size == nparams

    # ranks -> wsum, with the error model of step_fp64's wpair
    r = uo.centered_rank_exact(fit)
    r_err = U * ((r + 0.5) + np.abs(r))
    w = r[0::2] + r[1::2]
    w_err = r_err[0::2] + r_err[1::2] + U * np.abs(w)

    g, abs_sum, spread = sigma_grad_fp64(w, 0, pairs, seed, iteration,
                                         nparams, w_err=w_err)
    g_tol = sigma_grad_tol(abs_sum, pairs,
                           uo.grad_chunks(pairs, nparams)) + spread

    c = 0.5 * float(snes.lr_sigma) / float(pop_total)
    p = g * c
    p_tol = c * g_tol + 2.0 * U * np.abs(p)
    e = np.exp(p)
    e_tol = e * (p_tol + ULP)
    ref = sig0 * e
    ref_tol = sig0 * e_tol + U * np.abs(ref)

    lo = float(np.float32(snes.sigma_min))
    hi = float(np.float32(snes.sigma_max))
    flag = (np.abs(ref - lo) <= ref_tol) | (np.abs(ref - hi) <= ref_tol)
    new = np.clip(ref, lo, hi)
    tol = np.where((ref > lo) & (ref < hi), ref_tol, 0.0)
    return new, tol, flag
