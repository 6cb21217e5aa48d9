"""Float64 oracle of the CartPole kernels (CPU only, numpy).

A second reading of fiber_amd/csrc/ops/cartpole_kernels.hip, written from
the kernel source.  The physics is ``cart_physics`` operation by operation:
the same Horner polynomials for sin and cos (with their exact rational
coefficients), the same products and fmas, in float64.  Next to every value
runs a bound on ``|kernel's fp32 value - this value|``: an operation passes
its operands' bounds on by the triangle inequality and adds ``U`` times its
own result for the one fp32 rounding the kernel makes there (constants such
as 4/3 and the polynomial coefficients count one rounding too).  The bound
of a new-state component is therefore "fp32 roundings on its path x U x the
magnitudes involved"; what the functions return is that times ``SAFETY``,
the constant and the reasoning of rollout_oracle.py.

Divisions: the kernel uses true IEEE division (``__fdiv_rn``), one rounding
each.  ``1 / (mc + mp)`` is formed once per launch and multiplied in, so
the kernel's ``temp`` carries the rounding of that reciprocal and of the
product; both are counted.

The policy half is rollout_oracle's: ``make_policy`` and phases A to C of
``rollout_oracle.rollout``, run for one step on a zero environment to get
the action and whether it is decided.

A step of an environment is *decided* when its action is decided by that
margin rule and both ``| |x'| - x_thr |`` and ``| |th'| - th_thr |`` exceed
the bound of the new state: then no fp32 rounding in the kernel can change
the action or the termination.
"""

import collections

import numpy as np

from . import philox_ref
from . import rollout_oracle as R
from .rollout_oracle import SAFETY, U, Z_REL, make_policy  # noqa: F401

OBS, ENVS = 4, 64
C005 = np.float32(0.05)


def cart_array(gravity=9.8, masscart=1.0, masspole=0.1, length=0.5,
               force_mag=10.0, tau=0.02, x_threshold=2.4,
               theta_threshold=12 * 2 * np.pi / 360):
    """``ops.cartpole_params`` as a float32 numpy array."""
    return np.array([gravity, masscart, masspole, length, force_mag, tau,
                     x_threshold, theta_threshold], dtype=np.float32)


# ---- (value, bound) arithmetic: one fp32 rounding per operation -----------
def _rnd(v, e):
    return v, e + U * (np.abs(v) + e)


def _const(c):
    """A rational the kernel holds as the nearest fp32."""
    return c, U * abs(c)


def _mul(a, b):
    return _rnd(a[0] * b[0],
                np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1])


def _fma(a, b, c):
    return _rnd(a[0] * b[0] + c[0],
                np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1]
                + c[1])


def _div(a, b):
    v = a[0] / b[0]
    return _rnd(v, (a[1] + np.abs(v) * b[1]) / (np.abs(b[0]) - b[1]))


def _neg(a):
    return -a[0], a[1]


_S3, _S5, _S7 = _const(-1 / 6), _const(1 / 120), _const(-1 / 5040)
_C2, _C4, _C6, _C8 = (_const(-1 / 2), _const(1 / 24), _const(-1 / 720),
                      _const(1 / 40320))
_C43 = _const(4 / 3)
_ONE = (1.0, 0.0)


def _step_raw(state, action, cart, state_err):
    """cart_consts + cart_physics.  Returns (next[n][4], raw bound[n][4])."""
    s = np.asarray(state, dtype=np.float64)
    d = (np.zeros_like(s) if state_err is None
         else np.asarray(state_err, dtype=np.float64))
    g, mc, mp, l, force_mag, tau, _xt, _tt = [
        (float(c), 0.0) for c in np.asarray(cart, dtype=np.float32)]
    x, xd, th, thd = [(s[:, i], d[:, i]) for i in range(OBS)]
    # cart_consts
    inv_total = _div(_ONE, _rnd(mc[0] + mp[0], 0.0))
    pml = _mul(mp, l)
    mpt = _mul(mp, inv_total)
    pmlt = _mul(pml, inv_total)
    # cart_physics
    t2 = _mul(th, th)
    sp = _fma(t2, _fma(t2, _S7, _S5), _S3)
    sn = _fma(th, _mul(t2, sp), th)
    cs = _fma(t2, _fma(t2, _fma(t2, _fma(t2, _C8, _C6), _C4), _C2), _ONE)
    force = (np.where(np.asarray(action, bool), force_mag[0],
                      -force_mag[0]), 0.0)
    temp = _mul(_fma(_mul(pml, _mul(thd, thd)), sn, force), inv_total)
    num = _fma(_neg(cs), temp, _mul(g, sn))
    den = _mul(l, _fma(_neg(mpt), _mul(cs, cs), _C43))
    th_acc = _div(num, den)
    x_acc = _fma(_neg(_mul(pmlt, th_acc)), cs, temp)
    new = [_fma(tau, xd, x), _fma(tau, x_acc, xd), _fma(tau, thd, th),
           _fma(tau, th_acc, thd)]
    return (np.stack([v for v, _ in new], axis=-1),
            np.stack([np.broadcast_to(e, s.shape[:1]) for _, e in new],
                     axis=-1))


def _done(nxt, bound, cart):
    """(done, decided) of new states whose bound already has SAFETY."""
    x_thr, th_thr = float(cart[6]), float(cart[7])
    ax, ath = np.abs(nxt[:, 0]), np.abs(nxt[:, 2])
    return ((ax > x_thr) | (ath > th_thr),
            (np.abs(ax - x_thr) > bound[:, 0])
            & (np.abs(ath - th_thr) > bound[:, 2]))


def step(state, action, cart, state_err=None):
    """One step of ``state[n][4]`` under ``action[n]`` (bool, True pushes
    right).  Returns ``(next[n][4], bound[n][4], done[n], done_decided[n])``;
    ``bound`` has SAFETY, and ``state_err`` (optional) bounds the input."""
    cart = np.asarray(cart, dtype=np.float32)
    nxt, raw = _step_raw(state, action, cart, state_err)
    bound = SAFETY * raw
    return (nxt, bound) + _done(nxt, bound, cart)


def policy_step(pol, state, obs_mu, obs_nu, state_err=None):
    """(action[n], decided[n]) of ``pol`` for the states: phases A to C of
    rollout_oracle.rollout, one step on a zero environment.  That function
    takes states as float32, which moves a float64 one by up to U of it."""
    s = np.asarray(state, dtype=np.float64)
    err = U * np.abs(s) + (0.0 if state_err is None else state_err)
    ro = R.rollout(pol, obs_mu, obs_nu, np.zeros((OBS, OBS)), np.zeros(OBS),
                   s, 1, err)
    return ro.action[:, 0], ro.decided[:, 0]


def init_states(seed, iteration):
    """(s_0[64][4] float32, bound): ``0.05f * z`` of the FAM_TAG_ENV draw,
    z known to Z_REL between the device's libm and numpy's."""
    e = np.arange(ENVS, dtype=np.uint32)
    z = philox_ref.normal4(seed, iteration, e, np.uint32(0),
                           philox_ref.TAG_ENV, np.uint32(0))
    s0 = (C005 * z[:, :OBS].astype(np.float32)).astype(np.float32)
    return s0, np.abs(s0.astype(np.float64)) * (Z_REL + U)


Rollout = collections.namedtuple("Rollout", [
    "states",     # [E][H+1][4]  frozen once the environment has ended
    "state_err",  # [E][H+1][4]  bound (with SAFETY) while decided
    "alive",      # [E][H+1]     alive[e][t]: s_t is presented to the policy
    "decided",    # [E][H]       every step taken up to t is decided
    "step_decided",  # [E][H]    step t alone is, restarted from s_t as given
    "lengths",    # [E]          steps taken, the terminating one included
    "ended_by_x", "ended_by_th"])  # [E] the new state passed that threshold


def rollout(pol, obs_mu, obs_nu, cart, s0, horizon, s0_err=None):
    """The chained episode of every environment from ``s0[E][4]``."""
    cart = np.asarray(cart, dtype=np.float32)
    s = np.asarray(s0, dtype=np.float64)
    E, H = s.shape[0], int(horizon)
    delta = (np.zeros_like(s) if s0_err is None
             else np.asarray(s0_err, dtype=np.float64))
    out = Rollout(np.empty((E, H + 1, OBS)), np.empty((E, H + 1, OBS)),
                  np.zeros((E, H + 1), bool), np.zeros((E, H), bool),
                  np.ones((E, H), bool), np.zeros(E, int), np.zeros(E, bool), np.zeros(E, bool))
    alive = np.ones(E, bool)
    ok = np.ones(E, bool)
    for t in range(H + 1):
        out.states[:, t] = s
        out.state_err[:, t] = SAFETY * delta
        out.alive[:, t] = alive
        if t == H:
            break
        if alive.any():
            act, act_ok = policy_step(pol, s, obs_mu, obs_nu, delta)
            nxt, raw = _step_raw(s, act, cart, delta)
            done, done_ok = _done(nxt, SAFETY * raw, cart)
            ok &= ~alive | (act_ok & done_ok)
            act0, act0_ok = policy_step(pol, s, obs_mu, obs_nu)
            out.step_decided[:, t] = ~alive | (
                act0_ok & step(s, act0, cart)[3])
            out.lengths[:] += alive
            ending = alive & done
            out.ended_by_x[:] |= ending & (np.abs(nxt[:, 0]) > cart[6])
            out.ended_by_th[:] |= ending & (np.abs(nxt[:, 2]) > cart[7])
            s = np.where(alive[:, None], nxt, s)
            delta = np.where(alive[:, None], raw, delta)
            alive = alive & ~done
        out.decided[:, t] = ok
    return out


def member_rollout(theta, sigma, seed, iteration, horizon, member, obs_mu,
                   obs_nu, cart):
    """Block ``member`` (member_offset already added) of
    es_rollout_mlp_cartpole."""
    s0, s0_err = init_states(seed, iteration)
    z = philox_ref.noise_for_pair(seed, iteration, member // 2, R.NPARAMS)
    sgn = -float(sigma) if member % 2 else float(sigma)
    return rollout(make_policy(theta, sgn, z), obs_mu, obs_nu, cart, s0,
                   horizon, s0_err)


def obs_stats(rollouts):
    """What obs_stat[:8] accumulates for these members, as
    rollout_oracle.ObsStats: the states presented to the policy (``alive``),
    per dim.  A term passes at most ``horizon`` adds in its lane, 6 in the
    shuffle tree and 1 + 8 in cartpole_stat_reduce."""
    tot = [np.zeros(OBS) for _ in range(5)]
    n = 0
    for ro in rollouts:
        m = ro.alive[:, :-1, None]
        s = ro.states[:, :-1]
        d = ro.state_err[:, :-1]
        for acc, term in zip(tot, (s, s * s, np.abs(s), d,
                                   2.0 * np.abs(s) * d + d * d + U * s * s)):
            acc += (term * m).sum(axis=(0, 1))
        n += int(m.sum())
    assert len(rollouts) <= 256
    depth = rollouts[0].alive.shape[1] - 1 + 6 + 9
    return R.ObsStats(tot[0], tot[1], tot[2], max(n, depth), depth, tot[3],
                      tot[4])
