"""One-step-at-a-time checks of the MLP rollout loop at long horizons,
shared by tests/test_rollout_step.py (CPU) and
tests/gpu/test_rollout_step_gpu.py.  Everything here runs without a GPU and
nothing here is modified by a test.

The multi-step oracle comparison drops an episode at its first undecided
step and so compares nothing past a handful of steps.  Here the kernel's own
fp32 state at horizon h (``final_states`` of the ``_bc`` kernels) is the
start of ONE oracle step, compared with the kernel's state at h + 1: nothing
accumulates, the state bound is the one-step bound (under 1e-6), and an
undecided step is not skipped: the env step has two outcomes only, so the
kernel's state must be one of the two.  Derivations:
profiles/rollout_oracle.md, "One step at a time".
"""

import collections
import functools

import numpy as np

import rollout_oracle_cases as C
from fiber_amd.es import rollout_oracle as oracle

U = oracle.U
CELLS = [(k, m) for k in range(C.K) for m in range(C.M)]

# Horizons h of the (h, h + 1) launch pairs: both parities of h (the state
# double buffer), 49 and 50 where the multi-step decided share is 0, and
# 199, whose h + 1 is the engine's default horizon.
H_LIST = (8, 49, 50, 199)
H_TOP = max(H_LIST) + 1
# least share of the 64 envs of a (cell or member, h) whose step is decided
CAP = 0.90

# ---- input sets -------------------------------------------------------------
# "base": rollout_oracle_cases' eval-matrix inputs.  "clamp": the same
# thetas and environments with the variance of dims 0 and 1 on the floor
# that ESEngine.step puts under it (rstd = 9.95) and the mean of dim 1
# moved, so that the +-5 clamp of the normalised obs fires in both signs
# while dims 2 and 3 never reach it.
NU_FLOOR = np.float32(1e-2)
CLAMP_MU1 = np.float32(0.45)
SETS = ("base", "clamp")
CLAMP_HORIZONS = (1, 2, 3)          # multi-step comparison on "clamp"
CLAMP_STEP_H = 50                   # its one long h of the one-step check
STEP_CASES = tuple(("base", h) for h in H_LIST) + (("clamp", CLAMP_STEP_H),)


def inputs_torch(name, device="cpu"):
    thetas, mu, nu, A, B = C.inputs_torch("cpu")
    if name == "clamp":
        nu = nu.clone()
        mu = mu.clone()
        nu[:, 0:2] = float(NU_FLOOR)
        mu[:, 1] = float(CLAMP_MU1)
    else:
        assert name == "base"
    return [t.to(device).contiguous() for t in (thetas, mu, nu, A, B)]


@functools.lru_cache(maxsize=None)
def inputs_numpy(name):
    out = tuple(t.numpy().copy() for t in inputs_torch(name))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cell_policy(k):
    return oracle.make_policy(inputs_numpy("base")[0][k])


def cell_args(name, k, m):
    _th, mu, nu, A, B = inputs_numpy(name)
    return cell_policy(k), mu[k], nu[k], A[m], B[m]


@functools.lru_cache(maxsize=None)
def trajectory(name, k, m):
    """The oracle's own H_TOP-step rollout of cell (k, m): the source of
    the CPU conditions and of the stand-in kernels."""
    s0, s0_err = oracle.init_states(C.SEED, C.ITER)
    return oracle.rollout(*cell_args(name, k, m), s0, H_TOP, s0_err)


@functools.lru_cache(maxsize=None)
def clamp_cell(k, m, flip_step=None):
    """eval_cell of the "clamp" set through max(CLAMP_HORIZONS) steps."""
    th, mu, nu, A, B = inputs_numpy("clamp")
    return oracle.eval_cell(th[k], mu[k], nu[k], A[m], B[m], C.SEED, C.ITER,
                            max(CLAMP_HORIZONS), flip_step)


# ---- perturbed members ------------------------------------------------------
# One launch of POP = 4 members at member_offset 3 (members 3, 4, 5, 6: the
# pair (2, 3) is split, (4, 5) is whole, (6, 7) is split) per sigma, on
# rollout_oracle_cases.member_args().  The seed is the first of 100, 101, ..
# at which the oracle's own trajectory leaves at least CAP of every member's
# 64 envs decided at every h of MEMBER_H; the ones before it are listed in
# MEMBER_SEEDS_REJECTED as (seed, least share) with the share that ruled
# them out, and tests/test_rollout_step.py asserts both.  Seed 100 meets
# the cap at both sigmas (least shares 0.953 / 0.922 at sigma 0.05, 1.0 /
# 1.0 at sigma 4.0, for h = 50 / 199), so no seed was rejected.
MEMBER_OFFSET = 3
MEMBER_H = (50, 199)
MEMBER_H_TOP = max(MEMBER_H) + 1
MEMBER_SEEDS = {0.05: 100, 4.0: 100}
MEMBER_SEEDS_REJECTED = {0.05: (), 4.0: ()}


@functools.lru_cache(maxsize=None)
def member_policy(sigma, seed, member):
    from fiber_amd.es import philox_ref

    theta = C.member_args()[0]
    z = philox_ref.noise_for_pair(seed, C.ITER, member // 2, oracle.NPARAMS)
    sgn = -float(sigma) if member % 2 else float(sigma)
    return oracle.make_policy(theta, sgn, z)


def member_step_args(sigma, seed, member):
    _theta, mu, nu, A, B = C.member_args()
    return member_policy(sigma, seed, member), mu, nu, A, B


@functools.lru_cache(maxsize=None)
def member_trajectory(sigma, seed, member):
    s0, s0_err = oracle.init_states(seed, C.ITER)
    return oracle.rollout(*member_step_args(sigma, seed, member), s0,
                          MEMBER_H_TOP, s0_err)


def member_shares(sigma, seed):
    """Least decided share of the one-step restart over the launch's
    members, per h of MEMBER_H, from the oracle alone."""
    out = []
    for h in MEMBER_H:
        worst = 1.0
        for i in range(C.POP):
            member = MEMBER_OFFSET + i
            tr = member_trajectory(sigma, seed, member)
            st = one_step(member_step_args(sigma, seed, member),
                          tr.states[:, h].astype(np.float32))
            worst = min(worst, float(st.decided.mean()))
        out.append(worst)
    return out


# ---- the one-step check -------------------------------------------------------

OneStep = collections.namedtuple("OneStep", [
    "decided",    # [E] the oracle calls the step from final_h decided
    "main",       # Rollout, one step, the oracle's action
    "alt",        # Rollout, one step, the other action (flip_step=0)
    "x_raw"])     # [E][4] unclamped normalised obs of final_h, float64


def one_step(args, final_h):
    """One oracle step from the kernel's exact fp32 state ``final_h``
    [E][4] (so no s0_err), with both outcomes of the env step."""
    pol, mu, nu, A, B = args
    s = np.asarray(final_h, dtype=np.float32)
    main = oracle.rollout(pol, mu, nu, A, B, s, 1)
    alt = oracle.rollout(pol, mu, nu, A, B, s, 1, flip_step=0)
    assert (alt.action[:, 0] != main.action[:, 0]).all()
    mu64 = np.asarray(mu, dtype=np.float32).astype(np.float64)
    nu64 = np.asarray(nu, dtype=np.float32).astype(np.float64)
    x_raw = (s.astype(np.float64) - mu64) / np.sqrt(nu64 + oracle.C1EM4)
    return OneStep(main.decided[:, 0], main, alt, x_raw)


StateMatch = collections.namedtuple("StateMatch", [
    "ok",         # [E] final_h1 is the decided outcome / one of the two
    "took_alt",   # [E] an undecided step whose state is the other outcome
    "ratio"])     # [E] max_d |final_h1 - matched outcome| / state_err


def match_states(st, final_h1):
    """Every env is compared: where the step is decided, with the oracle's
    outcome; where it is not, with both outcomes, and it must lie within
    the bound of one."""
    f1 = np.asarray(final_h1, dtype=np.float32).astype(np.float64)
    r_main = (np.abs(f1 - st.main.states[:, 1])
              / st.main.state_err[:, 1]).max(-1)
    r_alt = (np.abs(f1 - st.alt.states[:, 1])
             / st.alt.state_err[:, 1]).max(-1)
    took_alt = ~st.decided & (r_alt < r_main)
    ratio = np.where(took_alt, r_alt, r_main)
    return StateMatch(ratio <= 1.0, took_alt, ratio)


def partial_bound(n_steps, s_max):
    """Bound on sum_d |partial_d| after ``n_steps`` steps: the thread of
    dim d adds 1[d == 0] - 0.1 s[d]^2 per step, |s| <= s_max."""
    return n_steps * (1.0 + oracle.OBS * oracle.C01 * s_max * s_max)


def reward_tol(st, took_alt, h, s_max):
    """Bound on |(episodes_{h+1} - episodes_h) - reward[:, 0]|.

    The kernel holds four per-dim running fp32 sums and adds them with
    three adds.  partial_d(h+1) = fl(partial_d(h) + r_d): U |partial_d(h+1)|
    per dim.  Each episode is ((p0 + p1) + p2) + p3: three adds, each
    rounding a partial sum that is at most sum_d |partial_d|, on both
    sides.  In all U * (P(h+1) + 3 P(h+1) + 3 P(h)) <= 7 U P(h+1) with
    P(n) = partial_bound(n, s_max).  Added to it is the oracle's own bound
    on the reward of one step from an exact state, return_tol[:, 0]."""
    one = np.where(took_alt, st.alt.return_tol[:, 0],
                   st.main.return_tol[:, 0])
    return one + 7.0 * U * partial_bound(h + 1, s_max)


def match_reward(st, sm, ep_h, ep_h1, h, s_max):
    """(|error|, tolerance) per env of the reward of step h: the episode
    difference of the two launches against the reward of the outcome the
    state was matched to."""
    want = np.where(sm.took_alt, st.alt.reward[:, 0], st.main.reward[:, 0])
    got = (np.asarray(ep_h1, dtype=np.float32).astype(np.float64)
           - np.asarray(ep_h, dtype=np.float32).astype(np.float64))
    return np.abs(got - want), reward_tol(st, sm.took_alt, h, s_max)


def clamp_condition(x_raw):
    """``x_raw`` [..., 4]: (some x above +5, some below -5, some dim that
    holds a clamped and an unclamped value) and the shares behind them."""
    x = np.asarray(x_raw).reshape(-1, oracle.OBS)
    hi, lo = x > 5.0, x < -5.0
    mixed = ((hi | lo).any(0) & (~(hi | lo)).any(0)).any()
    return (bool(hi.any()), bool(lo.any()), bool(mixed),
            hi.mean(0), lo.mean(0))


# ---- obs statistics at the production horizon ---------------------------------
STAT_H = (199, 200)


def stat_step_want(finals):
    """obs_stat_{h+1} - obs_stat_h is the state s_h of every env of every
    member, i.e. ``finals`` [POP][64][4] of the _bc sibling at h: (want[8],
    sum of |terms| [8]) in float64; the kernel squares in fp32, one
    rounding, U s^2 per term."""
    s = np.asarray(finals, dtype=np.float32).astype(np.float64).reshape(
        -1, oracle.OBS)
    want = np.concatenate([s.sum(0), (s * s).sum(0)])
    absw = np.concatenate([np.abs(s).sum(0), (s * s).sum(0)])
    return want, absw


def stat_step_tol(stat_h, stat_h1, absw, h, n_eps):
    """Tolerance [8] of obs_stat_{h+1} - obs_stat_h against stat_step_want.

    As obs_stats_tol: every fp32 add rounds by at most U of a partial sum
    that never exceeds the sum of |terms| below it, and a term passes
    through at most depth = (horizon - 1) + 6 + 8 adds.  The difference of
    two long accumulations carries the rounding of both: depth_h U abs_h +
    depth_{h+1} U abs_{h+1}, with abs_* the absolute sums of the two
    accumulations (not n_terms * U * ...).  The states between the launches'
    ends are not returned, so the absolute sums come from the kernel's
    sumsq slots: all their terms are positive, so the slot is its own
    absolute sum to within depth * U of itself, and for the sum slots
    sum |s| <= sqrt(n_terms * sum s^2) (Cauchy-Schwarz).  U * absw[4:] is
    the one rounding of each square of the new terms."""
    tol = np.zeros(2 * oracle.OBS)
    for stat, hor in ((stat_h, h), (stat_h1, h + 1)):
        depth = (hor - 1) + 6 + 8
        sq = np.asarray(stat, dtype=np.float64)[4:8] * (
            1.0 + 2.0 * depth * U)
        n_terms = float(n_eps * hor)
        tol += depth * U * np.concatenate([np.sqrt(n_terms * sq), sq])
    tol[4:] += U * absw[4:]
    return tol


# ---- stand-in kernels for the mutation checks -----------------------------------
DEFECTS = ("no_clamp", "clamp_4", "wrong_buffer", "reward_dropped")


def standin_step(args, s, s_prev, defect=None):
    """One step of a plain float64 stand-in "kernel" with at most one
    defect: (final_h1 float32 [E][4], reward of the step [E])."""
    pol, mu, nu, A, B = args
    mu, nu, A, B = (np.asarray(a, dtype=np.float32).astype(np.float64)
                    for a in (mu, nu, A, B))
    s = np.asarray(s, dtype=np.float32).astype(np.float64)
    x = (s - mu) / np.sqrt(nu + oracle.C1EM4)
    if defect == "clamp_4":
        x = np.clip(x, -4.0, 4.0)
    elif defect != "no_clamp":
        x = np.clip(x, -5.0, 5.0)
    xb = oracle.bf16_round(x)[0]
    h1 = oracle.bf16_round(np.tanh(xb @ pol.w1.T + pol.b1))[0]
    l0, l1 = oracle.logits_from_h1(pol, h1)
    asign = np.where(l1 > l0, 1.0, -1.0)
    # the state double buffer: the drive reads the buffer of step h - 1
    sd = np.asarray(s_prev, dtype=np.float64) if defect == "wrong_buffer" \
        else s
    snew = (oracle.C008 * np.tanh(sd @ A.T) + oracle.C097 * s
            + oracle.C005 * B * asign[:, None])
    r = (np.array([1.0, 0.0, 0.0, 0.0]) - oracle.C01 * snew * snew).sum(-1)
    if defect == "reward_dropped":
        r = np.zeros_like(r)
    return snew.astype(np.float32), r


def standin_check(args, tr, h, defect=None):
    """The whole one-step check on a stand-in kernel that follows the
    oracle trajectory ``tr`` up to h: (decided, states ok, reward ok)."""
    final_h = tr.states[:, h].astype(np.float32)
    final_h1, r = standin_step(args, final_h, tr.states[:, h - 1], defect)
    ep_h = tr.returns[:, h - 1].astype(np.float32)
    ep_h1 = (ep_h.astype(np.float64) + r).astype(np.float32)
    st = one_step(args, final_h)
    sm = match_states(st, final_h1)
    s_max = np.abs(tr.states[:, :h + 2]).max()
    err, tol = match_reward(st, sm, ep_h, ep_h1, h, s_max)
    return st.decided, sm.ok, err <= tol
