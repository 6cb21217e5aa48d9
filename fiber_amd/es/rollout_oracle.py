"""Per-episode float64 oracle of the MLP rollout step loop (CPU only).

A second, independent reading of ``rollout_steps`` in
fiber_amd/csrc/ops/es_kernels.hip, the loop that es_rollout_mlp,
es_eval_matrix and es_rollout_mlp_pairs inline.  It is written from the
kernel source and shares nothing with ``engine._reference_step``.

Everything is float64 except the roundings the kernel makes to bf16, which
are reproduced exactly: W1, W2, W3 when the policy is staged, the clamped
normalised obs ``x``, and ``h1``.  ``h2`` stays unrounded, biases stay as
given.  The Philox draws come from ``philox_ref``.

The policy reaches the environment only through ``asign = (l1 > l0)``.
While every action of an episode matches the kernel's, the kernel's state
trajectory equals this one to within fp32 rounding, about 1e-6 per step,
so an episode can be compared thousands of times more tightly than the
5e-2 mean-over-64 checks.  The oracle therefore also says, from its own
numbers alone, which steps are *decided*: those where no fp32 rounding
inside the kernel can turn the action.  The rule, per env and step:

* every value about to be rounded to bf16 has a distance to the nearest
  bf16 rounding midpoint.  ``x`` closer to one than the fp32 error of
  ``(s - mu) * rstd`` makes the step undecided;
* an ``h1`` value, or a perturbed weight ``theta + sgn*z``, closer to a
  midpoint than its fp32 error may round the other way in the kernel.  It
  adds ``ulp * sensitivity`` to a perturbation bound on ``l1 - l0``; for
  h1[j] the sensitivity is ``sum_i |w3[1][i]-w3[0][i]| * tanh'_i *
  |w2[i][j]|``.  tanh'_i is bounded by ``tanh_slope``: 1 - tanh^2 at the
  point nearest 0 that the pre-activation can reach, which is never above
  1.  With the plain bound tanh' <= 1 no sigma = 4.0 member is decided in
  all its envs: its saturated layers have sum |w3||w2| near 1000;
* the step is decided iff
  ``margin > SAFETY * (eps_logits + perturbation bound)``, where
  ``eps_logits`` is a worst-case fp32 bound on ``l1 - l0`` computed from
  the magnitudes of that very step;
* once a step is undecided, everything after it in that episode is too.

The constants are derived in profiles/rollout_oracle.md from the kernel's
arithmetic (fp32 accumulate in the MFMA, bf16 inputs, fast_tanh as
``1 - 2*rcp(exp2(x*TWO_LOG2E) + 1)``).  ``TANH_EMUL_ERR`` is the largest
``|float32 emulation of that formula - float64 tanh|`` measured on the
CPU by ``measure_tanh_emulation_error`` (1.83e-7, see that file); nothing
here comes from a GPU run.
"""

import collections

import numpy as np

from . import philox_ref

OBS, HID, ACT, ENVS = 4, 64, 2, 64
OFF_B1, OFF_W2, OFF_B2, OFF_W3, OFF_B3, NPARAMS = (
    256, 320, 4416, 4480, 4608, 4610)

U = 2.0 ** -24      # fp32 unit roundoff: one round-to-nearest operation
ULP = 2.0 ** -23    # largest relative spacing of fp32: "1 ulp" of a
                    # device function, relative to its result

# ---- fast_tanh ------------------------------------------------------------
# Largest |fp32 emulation - fp64 tanh|, exp2 and rcp emulated as correctly
# rounded: measure_tanh_emulation_error gives 1.831e-7 (the CPU test
# measures it again and checks that it does not exceed this).  Beyond
# |x| = 10 the emulation is exactly +-1 and the error falls under 1e-8, so
# the sigma = 4.0 members, whose pre-activations reach the hundreds, stay
# inside the measured range.
TANH_EMUL_ERR = 2.0e-7
# v_exp_f32 and v_rcp_f32 are documented to 1 ulp, not correctly rounded.
# t = 1 - 2/(e+1): dt/de * e*ULP = 2e/(e+1)^2 * ULP <= ULP/2, and 1 ulp of
# r = rcp(e+1) <= 1 moves t by at most 2*ULP.
TANH_HW_ERR = 0.5 * ULP + 2.0 * ULP
EPS_TANH = 4.0 * (TANH_EMUL_ERR + TANH_HW_ERR)

# ---- draws ------------------------------------------------------------
# z = sqrt(-2 log u0) * cos(2 pi u1).  The uniforms are exact integer
# arithmetic and identical on both sides.  With logf, sinf, cosf within
# 2 ulp and sqrtf correctly rounded: log 2 ulp, halved by the sqrt, + U for
# its rounding, + 2 ulp for cos/sin, + U for the product: under 4 ulp of z.
# The same allowance again for numpy's float32 routines, which the CPU test
# measures against a float64 Box-Muller.
Z_SIDE_ULPS = 4.0
Z_REL = 2.0 * Z_SIDE_ULPS * ULP

# ---- normalised obs -----------------------------------------------------
# x = (s - mu) * rsqrtf(nu + 1e-4f): U for the subtract, 2 ulp for rsqrtf,
# U/2 for the add under it (halved by the power -1/2), U for the product.
X_REL = 7.0 * U

# ---- accumulation lengths ----------------------------------------------
# fp32 sums of n terms in any order are within (n-1)*U*sum|terms| of the
# exact sum, to first order.  Layer 1: 4 non-zero products + bias.  Layer
# 2: 64 products + bias.  Logits: 64 fmas, the 2-level lane reduce, the
# 4 wave partials and b3.
N_L1 = 5
N_L2 = 65
N_LOGIT = 66

# The bounds above take every fp32 operation as round-to-nearest (error
# U).  The MFMA documents fp32 accumulation but not the rounding of its
# internal adds; if they truncate, each costs up to 2*U.  SAFETY covers
# that factor, so it is 2, not a tuned margin.
SAFETY = 2.0

C097 = float(np.float32(0.97))
C008 = float(np.float32(0.08))
C005 = float(np.float32(0.05))
C01 = float(np.float32(0.1))
C03 = float(np.float32(0.3))
C1EM4 = float(np.float32(1e-4))
TWO_LOG2E = float.fromhex("0x1.715476p+1")


def measure_tanh_emulation_error(dense=16.0, limit=1e4, n=2_000_001):
    """max |fp32 emulation of fast_tanh - fp64 tanh| on a dense grid over
    [-dense, dense] plus a log-spaced set from 1e-9 to ``limit``, both
    signs.  Each fp32 operation rounds once (IEEE), exp2 and the reciprocal
    are taken as correctly rounded; the 1-ulp allowance of the hardware
    units is TANH_HW_ERR."""
    x = np.concatenate([
        np.linspace(-dense, dense, n),
        np.geomspace(1e-9, limit, n // 4),
        -np.geomspace(1e-9, limit, n // 4),
    ]).astype(np.float32)
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        m = x * np.float32(TWO_LOG2E)                     # v_mul_f32
        e = np.exp2(m.astype(np.float64)).astype(np.float32)  # v_exp_f32
        ep1 = e + np.float32(1.0)                         # v_add_f32
        r = (1.0 / ep1.astype(np.float64)).astype(np.float32)  # v_rcp_f32
        # v_fma_f32(r, -2, 1): -2r is exact, one rounding
        t = (1.0 - 2.0 * r.astype(np.float64)).astype(np.float32)
    return float(np.max(np.abs(t.astype(np.float64)
                               - np.tanh(x.astype(np.float64)))))


def bf16_round(v):
    """Round float64 ``v`` to the nearest bf16 (ties to even), directly,
    not through float32.  Returns (rounded, distance of v to the nearest
    rounding midpoint of its binade, bf16 spacing in that binade)."""
    v = np.asarray(v, dtype=np.float64)
    _m, e = np.frexp(v)
    q = np.ldexp(1.0, e - 8)         # 8 significant bits
    k = v / q                        # exact: q is a power of two
    r = np.rint(k) * q               # rint rounds half to even
    dist = np.abs(k - np.floor(k) - 0.5) * q
    return r, dist, q


def tanh_slope(pre, radius):
    """Upper bound of tanh' on [pre - radius, pre + radius]: tanh' falls
    with |x|, so it is 1 - tanh^2 at the point of the interval nearest 0.
    Never above 1."""
    return 1.0 - np.tanh(np.maximum(np.abs(pre) - radius, 0.0)) ** 2


def bf16_other_neighbour(v, r, q):
    """The bf16 value on the other side of v from r: where the kernel lands
    if it rounds a near-midpoint value the other way."""
    return np.where(np.asarray(v) >= r, r + q, r - q)


Policy = collections.namedtuple("Policy", [
    "w1", "b1", "w2", "b2", "w3", "b3",          # float64, weights bf16
    "w1_flag", "w2_flag", "w3_flag",            # may round the other way
    "w1_q", "w2_q", "w3_q",                     # bf16 spacing per weight
    "b1_err", "b2_err", "b3_err",               # fp32 error of the biases
    "dw3", "w2_abs"])


def make_policy(theta, sgn=0.0, z=None):
    """The policy as the kernel stages it in LDS.  ``theta`` float32
    [NPARAMS]; for a perturbed member ``z`` is the pair's float32 noise and
    ``sgn`` is +-sigma.  The kernel forms ``theta[j] + sgn*z[j]`` in fp32
    (the compiler may fuse it into one fma) from its own z; the value here
    is the exact float64 sum from numpy's z, so it is known only to within
    ``|sgn z| * (Z_REL + U) + U*|w|``.  A weight closer than that to a bf16
    midpoint is flagged."""
    th = np.asarray(theta, dtype=np.float32).astype(np.float64)
    assert th.shape == (NPARAMS,)
    if z is None:
        w = th
        width = np.zeros_like(w)
    else:
        sz = float(np.float32(sgn)) * np.asarray(
            z, dtype=np.float32).astype(np.float64)
        w = th + sz
        width = np.abs(sz) * (Z_REL + U) + U * np.abs(w)

    def weights(lo, hi, shape):
        r, dist, q = bf16_round(w[lo:hi])
        flag = dist < width[lo:hi]
        return r.reshape(shape), flag.reshape(shape), q.reshape(shape)

    w1, f1, q1 = weights(0, OFF_B1, (HID, OBS))
    w2, f2, q2 = weights(OFF_W2, OFF_B2, (HID, HID))
    w3, f3, q3 = weights(OFF_W3, OFF_B3, (ACT, HID))
    dw3 = np.abs(w3[1] - w3[0])
    return Policy(
        w1, w[OFF_B1:OFF_W2], w2, w[OFF_B2:OFF_W3], w3, w[OFF_B3:],
        f1, f2, f3, q1, q2, q3,
        width[OFF_B1:OFF_W2], width[OFF_B2:OFF_W3], width[OFF_B3:],
        dw3, np.abs(w2))


def logits_from_h1(pol, h1):
    """(l0, l1) in float64 from bf16-valued h1[..., HID]: layer 2, its
    unrounded tanh, and the logits."""
    h2 = np.tanh(h1 @ pol.w2.T + pol.b2)
    l = h2 @ pol.w3.T + pol.b3
    return l[..., 0], l[..., 1]


Rollout = collections.namedtuple("Rollout", [
    "states",      # [E][H+1][4]  s_0 .. s_H
    "state_err",   # [E][H+1][4]  bound on |kernel - oracle| while decided
    "reward",      # [E][H]       sum_d (1[d==0] - 0.1 s_{t+1}[d]^2)
    "action",      # [E][H]       bool, l1 > l0
    "margin",      # [E][H]       |l1 - l0|
    "threshold",   # [E][H]       SAFETY * (eps_logits + perturbation)
    "decided",     # [E][H]       steps 0..t all decided
    "returns",     # [E][H]       returns[e][h-1]: episode return, horizon h
    "return_tol",  # [E][H]       bound on |kernel - oracle| of the above
    "h1",          # [E][H][64]   bf16 values
    "h1_alt",      # [E][H][64]   the other neighbour
    "h1_flag",     # [E][H][64]   near a midpoint: the kernel may take alt
    "x_flag",      # [E][H]       some x near a midpoint
    "policy"])


def rollout(pol, obs_mu, obs_nu, env_A, env_B, s0, horizon, s0_err=None,
            flip_step=None):
    """H steps of every env from ``s0`` [E][4].  ``flip_step=t`` negates
    the action of step t in every env: the envs are independent, so this
    is 64 single-action mutations at once (for the mutation tests)."""
    mu = np.asarray(obs_mu, dtype=np.float32).astype(np.float64)
    nu = np.asarray(obs_nu, dtype=np.float32).astype(np.float64)
    A = np.asarray(env_A, dtype=np.float32).astype(np.float64)
    B = np.asarray(env_B, dtype=np.float32).astype(np.float64)
    s = np.asarray(s0, dtype=np.float32).astype(np.float64)
    E, H = s.shape[0], int(horizon)
    rstd = 1.0 / np.sqrt(nu + C1EM4)
    absA = np.abs(A)
    delta = (np.zeros_like(s) if s0_err is None
             else np.asarray(s0_err, dtype=np.float64))
    one_d0 = np.array([1.0, 0.0, 0.0, 0.0])
    # C05B is rounded once in the kernel (0.05f * eB_d), then * +-1 exactly
    c05b = C005 * B

    out = Rollout(
        np.empty((E, H + 1, OBS)), np.empty((E, H + 1, OBS)),
        np.empty((E, H)), np.empty((E, H), bool), np.empty((E, H)),
        np.empty((E, H)), np.empty((E, H), bool), np.empty((E, H)),
        np.empty((E, H)), np.empty((E, H, HID)), np.empty((E, H, HID)),
        np.empty((E, H, HID), bool), np.empty((E, H), bool), pol)
    out.states[:, 0] = s
    out.state_err[:, 0] = delta
    racc = np.zeros((E, OBS))        # the kernel's 4 per-dim partials
    racc_err = np.zeros((E, OBS))
    alive = np.ones(E, bool)

    for t in range(H):
        # ---- phase A: normalised, clamped obs, rounded to bf16 ---------
        x_raw = (s - mu) * rstd
        xb, x_dist, _ = bf16_round(np.clip(x_raw, -5.0, 5.0))
        x_width = X_REL * np.abs(x_raw) + rstd * delta
        x_flag = (x_dist < x_width).any(axis=1)
        # ---- phase B: h1 = bf16(tanh(W1 x + b1)) -----------------------
        t1 = xb[:, None, :] * pol.w1[None, :, :]          # [E][64][4]
        pre1 = t1.sum(-1) + pol.b1
        e1 = (N_L1 * U * (np.abs(t1).sum(-1) + np.abs(pol.b1))
              + pol.b1_err
              + (np.abs(xb)[:, None, :] * (pol.w1_flag * pol.w1_q)).sum(-1))
        h1_raw = np.tanh(pre1)
        h1, h1_dist, h1_q = bf16_round(h1_raw)
        h1_flag = h1_dist < EPS_TANH + e1 * tanh_slope(pre1, e1)
        # ---- phase C: h2 unrounded, logits -----------------------------
        t2 = h1[:, None, :] * pol.w2[None, :, :]          # [E][64][64]
        pre2 = t2.sum(-1) + pol.b2
        e2 = N_L2 * U * (np.abs(t2).sum(-1) + np.abs(pol.b2)) + pol.b2_err
        # the most that other-way roundings (flagged h1, flagged W2) can
        # move each layer-2 pre-activation, and through it l1 - l0
        shift2 = ((h1_flag * h1_q) @ pol.w2_abs.T
                  + np.abs(h1) @ (pol.w2_flag * pol.w2_q).T)
        slope2 = tanh_slope(pre2, shift2 + e2)
        pert = (pol.dw3 * slope2 * shift2).sum(-1)
        h2 = np.tanh(pre2)
        h2_err = EPS_TANH + e2 * slope2
        t3 = h2[:, None, :] * pol.w3[None, :, :]          # [E][2][64]
        logits = t3.sum(-1) + pol.b3
        l_err = ((np.abs(pol.w3)[None] * h2_err[:, None, :]).sum(-1)
                 + N_LOGIT * U * (np.abs(t3).sum(-1) + np.abs(pol.b3))
                 + pol.b3_err)
        pert = pert + (np.abs(h2)[:, None, :]
                       * (pol.w3_flag * pol.w3_q)).sum((-1, -2))
        margin = np.abs(logits[:, 1] - logits[:, 0])
        thr = SAFETY * (l_err.sum(-1) + pert)
        act = logits[:, 1] > logits[:, 0]
        if flip_step == t:
            act = ~act
        alive = alive & ~x_flag & (margin > thr)
        # ---- phase D2: env step and reward -----------------------------
        asign = np.where(act, 1.0, -1.0)
        ts = A[None, :, :] * s[:, None, :]                # [E][d][e]
        drive = ts.sum(-1)
        drive_err = OBS * U * np.abs(ts).sum(-1) + delta @ absA.T
        th = np.tanh(drive)
        p97 = C097 * s
        inner = C008 * th + p97                           # the fmaf
        snew = inner + c05b * asign[:, None]
        delta = (C097 * delta + C008 * (EPS_TANH + drive_err)
                 + U * (np.abs(p97) + np.abs(inner) + np.abs(c05b)
                        + np.abs(snew)))
        r = one_d0 - C01 * snew * snew
        # (0.1f*s)*s, two roundings, then 1 - p, fused or not
        r_err = (2.0 * C01 * np.abs(snew) * delta + C01 * delta * delta
                 + 3.0 * U * C01 * snew * snew + U * np.abs(r))
        racc = racc + r
        racc_err = racc_err + r_err + U * np.abs(racc)
        s = snew

        out.states[:, t + 1] = s
        out.state_err[:, t + 1] = delta
        out.reward[:, t] = r.sum(-1)
        out.action[:, t] = act
        out.margin[:, t] = margin
        out.threshold[:, t] = thr
        out.decided[:, t] = alive
        # the episode is the sum of its 4 per-dim partials: 3 fp32 adds
        out.returns[:, t] = racc.sum(-1)
        out.return_tol[:, t] = (racc_err.sum(-1)
                                + 3.0 * U * np.abs(racc).sum(-1))
        out.h1[:, t] = h1
        out.h1_alt[:, t] = bf16_other_neighbour(h1_raw, h1, h1_q)
        out.h1_flag[:, t] = h1_flag
        out.x_flag[:, t] = x_flag
    return out


def init_states(seed, iteration):
    """(s_0 [ENVS][4] float32, bound on |kernel's s_0 - it|): 0.3f * z per
    env, z known to Z_REL between the device's libm and numpy's."""
    s0 = philox_ref.env_init_state(seed, iteration, ENVS)
    assert s0.dtype == np.float32
    return s0, np.abs(s0.astype(np.float64)) * Z_REL


def eval_cell(theta, obs_mu, obs_nu, env_A, env_B, seed, iteration,
              horizon, flip_step=None):
    """One cell of es_eval_matrix: the unperturbed ``theta``."""
    s0, s0_err = init_states(seed, iteration)
    return rollout(make_policy(theta), obs_mu, obs_nu, env_A, env_B, s0,
                   horizon, s0_err, flip_step)


def member_rollout(theta, sigma, seed, iteration, horizon, member, obs_mu,
                   obs_nu, env_A, env_B):
    """Block ``member`` (member_offset already added) of es_rollout_mlp:
    pair member//2, +sigma for even members, -sigma for odd ones."""
    s0, s0_err = init_states(seed, iteration)
    z = philox_ref.noise_for_pair(seed, iteration, member // 2, NPARAMS)
    sgn = -float(sigma) if member % 2 else float(sigma)
    return rollout(make_policy(theta, sgn, z), obs_mu, obs_nu, env_A, env_B,
                   s0, horizon, s0_err)


def fitness_of(ro, horizon):
    """(mean return over the envs at ``horizon``, bound on |kernel's
    fitness - it|).  The kernel sums the 64 fp32 returns in a 6-level
    shuffle tree, each value passing 6 adds, and divides by 64 exactly."""
    ep = ro.returns[:, horizon - 1]
    tol = (ro.return_tol[:, horizon - 1].mean()
           + 6.0 * U * np.abs(ep).mean())
    return float(ep.mean()), float(tol)


def member_fitness(theta, sigma, seed, iteration, horizon, member_offset,
                   index, obs_mu, obs_nu, env_A, env_B):
    """fitness[index] of es_rollout_mlp launched at ``member_offset``:
    (value, tolerance, decided-through-horizon for all 64 envs, rollout)."""
    ro = member_rollout(theta, sigma, seed, iteration, horizon,
                        member_offset + index, obs_mu, obs_nu, env_A, env_B)
    fit, tol = fitness_of(ro, horizon)
    return fit, tol, bool(ro.decided[:, horizon - 1].all()), ro


ObsStats = collections.namedtuple("ObsStats", [
    "sum", "sumsq",        # [4] float64, over members, envs and t < horizon
    "abs_sum",             # [4] sum |s|; sumsq is its own sum of |terms|
    "n_terms",             # terms per slot
    "depth",               # most fp32 adds any one term passes through
    "sum_err", "sumsq_err"])  # [4] summed per-state bounds


def obs_stats(rollouts, horizon):
    """What obs_stat[:8] accumulates for these members: the states
    s_0 .. s_{horizon-1} of every env, per dim.  ``sum_err`` / ``sumsq_err``
    add up the per-state bounds (state_err, and 2|s|*err + err^2 + U*s^2
    for the square, which the kernel rounds once)."""
    tot = [np.zeros(OBS) for _ in range(5)]
    n = 0
    for ro in rollouts:
        s = ro.states[:, :horizon]
        d = ro.state_err[:, :horizon]
        for acc, term in zip(tot, (s, s * s, np.abs(s), d,
                                   2.0 * np.abs(s) * d + d * d + U * s * s)):
            acc += term.sum(axis=(0, 1))
        n += s.shape[0] * s.shape[1]
    # a thread adds its env's `horizon` states in sequence, a 6-level
    # shuffle tree adds the 64 envs, and obs_stat_reduce adds the members:
    # one per thread up to 256 of them, then an 8-level LDS tree
    assert len(rollouts) <= 256
    depth = (horizon - 1) + 6 + 8
    return ObsStats(tot[0], tot[1], tot[2], n, depth, tot[3], tot[4])


def obs_stats_tol(st):
    """Per-slot tolerance [8] for obs_stat[:8]: every fp32 add rounds by at
    most U of a partial sum that never exceeds sum(|terms|), and a term
    passes through at most ``depth`` adds on its way to the slot; plus the
    summed state bounds.  ``depth`` is 16 or 17 here against n_terms in
    the hundreds, so this is well inside n_terms * U * sum(|terms|), the
    form of test_obs_stat_reduce_matches_per_member_sums: with that one the
    sums of two dims that lie 0.9 apart would pass for each other."""
    assert st.depth <= st.n_terms
    return np.concatenate([st.depth * U * st.abs_sum + st.sum_err,
                           st.depth * U * st.sumsq + st.sumsq_err])


def find_decided_launches(theta, sigma, horizon, pop, obs_mu, obs_nu, env_A,
                          env_B, seeds, offsets, iteration=0, want=1):
    """CPU search for launches of ``pop`` members whose 64 envs are all
    decided through ``horizon``: up to ``want`` (seed, member_offset)."""
    found = []
    for seed in seeds:
        for off in offsets:
            if all(member_fitness(theta, sigma, seed, iteration, horizon,
                                  off, i, obs_mu, obs_nu, env_A, env_B)[2]
                   for i in range(pop)):
                found.append((seed, off))
                if len(found) >= want:
                    return found
    return found
