"""Float64 oracle of the update half of an ES iteration (CPU only).

The rollout half has ``rollout_oracle``; this is its counterpart for what
turns fitness into a new ``theta``: the Box-Muller draws of ``fam_normal4``
(fiber_amd/csrc/ops/philox.h), ``es_grad`` / ``es_grad_reduce`` and
``centered_rank`` (es_kernels.hip), the chunk split of ``launch_grad``
(bindings.cpp), and the torch lines that ``ESEngine.step``,
``ConvESEngine.step`` and ``ESPopulation.step`` share.  It is written from
those sources and uses numpy only.

Every function returns float64 together with what a tolerance needs
(``abs_sum``, or a tolerance per element).  The derivations are in
profiles/update_oracle.md; ``U`` is one fp32 rounding, ``ULP`` one ulp of a
device function, as in ``rollout_oracle``.
"""

import numpy as np

from . import philox_ref
from .rollout_oracle import U, ULP, Z_SIDE_ULPS

_INV32 = np.float32(2.3283064365386963e-10)   # 2^-32
_TWOPI = np.float32(6.2831853071795864769)
C1EM2 = float(np.float32(1e-2))               # clamp_min(1e-2) on fp32


# ---- draws --------------------------------------------------------------

def draw_arguments(k0, k1, c0, c1, c2):
    """What ``fam_normal4`` feeds to logf and cosf/sinf, in the device's own
    float32 operations: ``(u0, u2, ang0, ang1)`` with ``u = (float(x) + 1) *
    2^-32`` and ``ang = twopi * u``.  u32 -> f32, the add and the product by
    twopi round once each, the product by 2^-32 is exact; numpy rounds them
    as the device does, so these arrays are the device's bits."""
    x = philox_ref.philox4x32_10(k0, k1, c0, c1, c2, np.uint32(0))
    u = [(xi.astype(np.float32) + np.float32(1.0)) * _INV32 for xi in x]
    return u[0], u[2], _TWOPI * u[1], _TWOPI * u[3]


def normals_fp64(k0, k1, c0, c1, c2):
    """Box-Muller in float64 from the float32 arguments of ``fam_normal4``:
    [..., 4].  Only log, sqrt, sin, cos and the final product are float64
    (``-2 *`` is exact in either), so the draws share their arguments with
    the device and a relative bound holds where cos or sin is near zero."""
    u0, u2, a0, a1 = draw_arguments(k0, k1, c0, c1, c2)
    a0 = a0.astype(np.float64)
    a1 = a1.astype(np.float64)
    r0 = np.sqrt(-2.0 * np.log(u0.astype(np.float64)))
    r1 = np.sqrt(-2.0 * np.log(u2.astype(np.float64)))
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0),
                     r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)


def rel_err(got, want):
    """|got - want| / |want| per element; a ``want`` of exactly 0 (u0 = 1)
    allows only 0."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    diff = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = diff / np.abs(want)
    return np.where(want == 0.0, np.where(diff == 0.0, 0.0, np.inf), r)


def param_index(nparams, jb=None):
    """Parameter indices covered by the parameter blocks ``jb`` (block jb
    holds 4*jb .. 4*jb+3), the ragged tail cut at ``nparams``."""
    if jb is None:
        return np.arange(nparams, dtype=np.int64)
    j = (np.asarray(jb, dtype=np.int64)[:, None] * 4
         + np.arange(4, dtype=np.int64)).reshape(-1)
    return j[j < nparams]


def noise_fp64(seed, iteration, pair, nparams, jb=None):
    """The eps vector of one antithetic pair in float64: ``nparams`` values,
    or with ``jb`` the values at ``param_index(nparams, jb)``."""
    if jb is None:
        jb = np.arange((nparams + 3) // 4, dtype=np.uint32)
    jb = np.asarray(jb)
    keep = (jb.astype(np.int64)[:, None] * 4 + np.arange(4)).reshape(-1)
    jb = jb.astype(np.uint32)
    z = normals_fp64(np.uint32(int(seed) & 0xFFFFFFFF),
                     np.uint32(int(iteration) & 0xFFFFFFFF),
                     np.uint32(pair) * np.ones_like(jb), jb,
                     philox_ref.TAG_NOISE)
    return z.reshape(-1)[keep < nparams]


# ---- gradient -------------------------------------------------------------

def grad_chunks(pairs, nparams):
    """``grad_chunks`` of bindings.cpp."""
    bx = ((nparams + 3) // 4 + 255) // 256
    if pairs < 64:
        return 1
    return 4 if bx >= 32 else 32


def grad_per_chunk(pairs, nparams):
    chunks = grad_chunks(pairs, nparams)
    return (pairs + chunks - 1) // chunks


def grad_fp64(w, pair_begin, pair_end, seed, iteration, nparams, jb=None,
              w_err=None):
    """``(g, abs_sum)``: ``g[j] = sum_k w[k] z_k[j]`` over the pairs
    ``pair_begin <= k < pair_end`` and ``abs_sum[j] = sum_k |w[k] z_k[j]|``,
    at ``param_index(nparams, jb)``.  ``w`` is indexed by the pair number,
    like the kernel's ``wpair``; nothing outside the range is read.  With
    ``w_err`` (a bound on each weight's own error) a third array
    ``sum_k w_err[k] |z_k[j]|`` is returned."""
    w = np.asarray(w).astype(np.float64)
    n = param_index(nparams, jb).size
    g = np.zeros(n)
    abs_sum = np.zeros(n)
    spread = np.zeros(n)
    for k in range(int(pair_begin), int(pair_end)):
        z = noise_fp64(seed, iteration, k, nparams, jb)
        t = w[k] * z
        g += t
        abs_sum += np.abs(t)
        if w_err is not None:
            spread += w_err[k] * np.abs(z)
    if w_err is not None:
        return g, abs_sum, spread
    return g, abs_sum


def grad_tol(abs_sum, pairs, chunks):
    """Bound on |es_grad - grad_fp64|: the draws' Z_SIDE_ULPS ulp, one
    rounding per accumulate (``acc += w*z`` contracts to an fma) over the
    at most ``per_chunk`` pairs of a chunk, and the ``chunks`` adds of
    es_grad_reduce."""
    per_chunk = (pairs + chunks - 1) // chunks
    return (Z_SIDE_ULPS * ULP + (per_chunk + chunks) * U) * np.asarray(
        abs_sum, dtype=np.float64)


# ---- centered rank ------------------------------------------------------

def ranks_exact(f):
    """Integer rank of every member: the number of members that are smaller,
    or equal with a lower index.  -0 equals +0."""
    f = np.asarray(f, dtype=np.float32).reshape(-1)
    assert not np.isnan(f).any()
    key = f + np.float32(0.0)            # -0 + 0 = +0
    order = np.lexsort((np.arange(f.size), key))   # by value, then index
    ranks = np.empty(f.size, dtype=np.int64)
    ranks[order] = np.arange(f.size, dtype=np.int64)
    return ranks


def centered_rank_exact(f):
    """``rank / (n - 1) - 0.5`` in float64.  The kernels round the division
    once (correctly) and the subtraction once: 2*U absolute covers both."""
    r = ranks_exact(f)
    if r.size < 2:
        raise ValueError("centered rank needs at least 2 members")
    return r.astype(np.float64) / (r.size - 1) - 0.5


RANK_TOL = 2.0 * U


def ranks_from_centered(c, n):
    """The integer ranks behind fp32 centered ranks ``c``: RANK_TOL * (n-1)
    is far below 1/2 for every n the O(n^2) and sort paths are used at."""
    assert RANK_TOL * (n - 1) < 0.25
    return np.rint((np.asarray(c, dtype=np.float64) + 0.5)
                   * (n - 1)).astype(np.int64)


# ---- one update step ------------------------------------------------------

def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def step_fp64(state, fitness, obs_stat, cfg, seed, iteration, nparams,
              pair_range=None):
    """One ``step()`` in float64 from the fp32 pre-step ``state`` (theta,
    adam_m, adam_v, t_step and, for the MLP engines, obs_sum, obs_sumsq,
    obs_count) and the device's own fp32 ``fitness`` of the whole
    population and ``obs_stat[9]`` (None for the conv engine).  ``cfg``
    carries sigma, lr, adam_beta1, adam_beta2, adam_eps.  ``pair_range`` is
    the shard's ``(pair_begin, pair_end)``, by default all pairs.

    Returns ``(new, tol, flags)``: the new state, a bound per element on
    |device - new| for every field, and ``flags["obs_nu_clamp"]``, true
    where the reference variance is within its tolerance of the 1e-2 clamp
    (there ``obs_nu`` may land on either side and is not comparable).

    Tolerances: first-order propagation of each input bound through the
    formula plus U per fp32 operation torch performs; a Python scalar
    entering a tensor operation is rounded to fp32 first (one U), and a
    division counts 2 U (it may be lowered to reciprocal and multiply).
    Where first order is not enough (the square root and the quotient of
    Adam at a coordinate whose gradient is within its tolerance of 0) the
    bound is taken over the interval instead."""
    fit = np.asarray(fitness, dtype=np.float32).reshape(-1)
    pop_total = fit.size
    if pair_range is None:
        pair_range = (0, pop_total // 2)
    pb, pe = pair_range

    # ranks -> wpair.  rank/(n-1) rounds once (relative to the quotient q
    # in [0, 1]), q - 0.5 once more; the subtraction of the two ranks once.
    r = centered_rank_exact(fit)
    r_err = U * ((r + 0.5) + np.abs(r))
    w = r[0::2] - r[1::2]
    w_err = r_err[0::2] + r_err[1::2] + U * np.abs(w)

    g, abs_sum, spread = grad_fp64(w, pb, pe, seed, iteration, nparams,
                                   w_err=w_err)
    pairs = pe - pb
    g_tol = grad_tol(abs_sum, pairs, grad_chunks(pairs, nparams)) + spread

    # grad /= float(pop_total) * sigma: the scalar to fp32, the division
    scale = float(pop_total) * float(cfg.sigma)
    g = g / scale
    g_tol = g_tol / scale + 3.0 * U * np.abs(g)

    b1, b2 = float(cfg.adam_beta1), float(cfg.adam_beta2)
    lr, eps = float(cfg.lr), float(cfg.adam_eps)
    t = int(state["t_step"]) + 1
    m0, v0, th0 = _f64(state["adam_m"]), _f64(state["adam_v"]), _f64(
        state["theta"])

    # adam_m.mul_(b1).add_(grad, alpha=1-b1): b1 -> fp32, the product;
    # alpha -> fp32, alpha*grad, the add
    m = b1 * m0 + (1.0 - b1) * g
    m_tol = ((1.0 - b1) * g_tol + 2.0 * U * np.abs(b1 * m0)
             + 2.0 * U * np.abs((1.0 - b1) * g) + U * np.abs(m))
    # adam_v.mul_(b2).addcmul_(grad, grad, value=1-b2): value -> fp32,
    # grad*grad, value*(..), the add
    v = b2 * v0 + (1.0 - b2) * g * g
    v_tol = ((1.0 - b2) * (2.0 * np.abs(g) * g_tol + g_tol * g_tol)
             + 2.0 * U * np.abs(b2 * v0)
             + 3.0 * U * (1.0 - b2) * g * g + U * np.abs(v))
    # mhat, vhat: the divisor -> fp32, the division
    d1, d2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    mhat, vhat = m / d1, v / d2
    mhat_tol = m_tol / d1 + 3.0 * U * np.abs(mhat)
    vhat_tol = v_tol / d2 + 3.0 * U * np.abs(vhat)
    # vhat.sqrt() + eps: sqrt is concave, so the largest move is downwards
    s = np.sqrt(vhat)
    s_tol = s - np.sqrt(np.maximum(vhat - vhat_tol, 0.0)) + U * s
    den = s + eps
    den_tol = s_tol + U * eps + U * den
    den_lo = den - den_tol
    # lr * mhat: lr -> fp32, the product
    num = lr * mhat
    num_tol = lr * mhat_tol + 2.0 * U * np.abs(num)
    upd = num / den
    with np.errstate(divide="ignore", invalid="ignore"):
        upd_tol = np.where(
            den_lo > 0.0,
            num_tol / den_lo + np.abs(num) * den_tol / (den * den_lo)
            + 2.0 * U * np.abs(upd),
            np.inf)
    theta = th0 + upd
    theta_tol = upd_tol + U * np.abs(theta)

    new = {"theta": theta, "adam_m": m, "adam_v": v, "t_step": t}
    tol = {"theta": theta_tol, "adam_m": m_tol, "adam_v": v_tol}
    flags = {}

    if obs_stat is not None:
        st = _f64(obs_stat).reshape(-1)
        n = (st.size - 1) // 2
        osum = _f64(state["obs_sum"]).reshape(-1) + st[:n]
        osq = _f64(state["obs_sumsq"]).reshape(-1) + st[n:2 * n]
        cnt = _f64(state["obs_count"]).reshape(-1) + st[2 * n:]
        osum_tol, osq_tol, cnt_tol = (U * np.abs(osum), U * np.abs(osq),
                                      U * np.abs(cnt))
        c = np.maximum(cnt, 1.0)
        c_tol = np.where(cnt > 1.0, cnt_tol, 0.0)
        mu = osum / c
        mu_tol = (osum_tol + np.abs(mu) * c_tol) / c + 2.0 * U * np.abs(mu)
        q = osq / c
        q_tol = (osq_tol + np.abs(q) * c_tol) / c + 2.0 * U * np.abs(q)
        # obs_mu ** 2 is one product
        sq_tol = 2.0 * np.abs(mu) * mu_tol + mu_tol * mu_tol + U * mu * mu
        var = q - mu * mu
        var_tol = q_tol + sq_tol + U * np.abs(var)
        flags["obs_nu_clamp"] = np.abs(var - C1EM2) <= var_tol
        nu = np.maximum(var, C1EM2)
        nu_tol = np.where(var > C1EM2, var_tol, 0.0)
        new.update(obs_sum=osum, obs_sumsq=osq, obs_count=cnt, obs_mu=mu,
                   obs_nu=nu)
        tol.update(obs_sum=osum_tol, obs_sumsq=osq_tol, obs_count=cnt_tol,
                   obs_mu=mu_tol, obs_nu=nu_tol)
    return new, tol, flags
