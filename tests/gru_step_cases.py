"""One-step-at-a-time checks of the GRU rollout kernel at depth, under
saturation and under the clamp, shared by tests/test_gru_step.py (CPU) and
tests/gpu/test_gru_step_gpu.py.  Everything here runs without a GPU and
nothing here is modified by a test.

The comparison is the restart scheme of tests/gpu/test_gru_gpu.py: the
kernel's own fp32 ``(state, hidden)`` at horizon h starts ONE step of
``gru_oracle``, which is compared with the kernel's ``(state, hidden)`` at
h + 1.  Nothing accumulates, so the tolerances of ``gru_oracle.cell`` and
``env_step`` are used as they are.  A "run" below is what one launch with
``return_final=True`` returns, as numpy arrays: ``(fitness[pop], obs_stat[9],
final_state[pop][64][4], final_hidden[pop][64][64])``.  The GPU tests feed
``compare_pair`` with the kernel's runs, the CPU tests with the runs of a
plain float64 stand-in that carries one defect at a time.  Derivations and
figures: profiles/gru.md, "One step at a time, at depth".
"""

import collections
import functools

import numpy as np

from fiber_amd.es import gru_oracle as G
from fiber_amd.es import philox_ref

ENVS = 64
WORLD_SEED, ITER = 4321, 3      # the ``world`` of tests/gpu/test_gru_gpu.py
OFFSET, POP = 2, 4              # members 2, 3, 4, 5: two whole pairs
MEMBERS = tuple(range(OFFSET, OFFSET + POP))
CAP = 0.90                      # least decided share per (member, h)

# horizons h of the (h, h + 1) launch pairs: both parities of the h double
# buffer, and 199, whose h + 1 is the engine's default horizon
H_DEEP = (8, 49, 50, 199)
H_CLAMP = (1, 2, 50)
H_TOP = 200                     # every step of one episode: h = 0 .. 199
H_MASK = (2, 3)
H_SERVING = (0, 7, 50, 199)
MASKS = tuple(range(16))

# ---- input sets -------------------------------------------------------------
# "clamp": the variance of dims 0 and 1 on the floor that the engines put
# under it (rstd = 9.95), and the mean of dim 1 moved, so that the +-5 clamp
# of the normalised obs fires in both signs in those dims at every h of
# H_CLAMP while dims 2 and 3 never reach it.
NU_FLOOR = np.float32(1e-2)
CLAMP_MU1 = np.float32(0.45)

Case = collections.namedtuple("Case", [
    "name", "theta", "mu", "nu", "A", "B", "sigma", "seed", "horizons"])

# name: (theta scale, sigma, clamp normaliser, horizons)
_SPEC = {
    "base0": (1.0, 0.0, False, H_DEEP),
    "base": (1.0, 0.05, False, H_DEEP),
    "wide": (1.0, 4.0, False, H_DEEP),
    "saturated": (8.0, 0.05, False, H_DEEP),
    "clamp": (1.0, 0.05, True, H_CLAMP),
}
SETS = tuple(_SPEC)

# The launch seed (noise and env init states) of a set is the first of
# WORLD_SEED, WORLD_SEED + 1, .. at which gru_oracle.rollout leaves at least
# CAP of every member's 64 envs decided at every checked h.  Seeds before it
# are listed as (seed, least share), with the share that ruled them out;
# tests/test_gru_step.py asserts both.  4321 meets the cap on every set
# (least shares in profiles/gru.md), so none was rejected.
SEEDS = {name: WORLD_SEED for name in SETS}
SEEDS_REJECTED = {name: () for name in SETS}

# one launch of 2 members far from pair 0 (pair = member >> 1 = 16383)
FAR_OFFSET, FAR_POP, FAR_H = 32766, 2, 8


@functools.lru_cache(maxsize=None)
def world():
    """theta, mu, nu, env_A, env_B of test_gru_gpu.py's ``world``, numpy."""
    from fiber_amd.es import init_theta_gru
    from fiber_amd.es.engine import make_env_params

    A, B = (t.numpy() for t in make_env_params(WORLD_SEED, "cpu"))
    mu = np.array([0.05, -0.1, 0.02, 0.0], dtype=np.float32)
    nu = np.array([0.3, 0.5, 0.2, 0.4], dtype=np.float32)
    out = (init_theta_gru(WORLD_SEED, "cpu").numpy(), mu, nu, A, B)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(name, seed=None):
    scale, sigma, clamp, horizons = _SPEC[name]
    theta, mu, nu, A, B = world()
    theta = (theta * np.float32(scale)).astype(np.float32)
    if clamp:
        mu, nu = mu.copy(), nu.copy()
        nu[0:2] = NU_FLOOR
        mu[1] = CLAMP_MU1
    for a in (theta, mu, nu):
        a.setflags(write=False)
    return Case(name, theta, mu, nu, A, B, sigma,
                SEEDS[name] if seed is None else seed, horizons)


_POLICIES = {}


def policy_for(c, member):
    """The perturbed policy of ``member`` as the kernel stages it; kept for
    the named sets, whose inputs never change."""
    key = (c.name, c.seed, member)
    if key in _POLICIES:
        return _POLICIES[key]
    z = philox_ref.noise_for_pair(c.seed, ITER, member // 2, G.GRU_NPARAMS)
    pol = G.make_policy(c.theta, -c.sigma if member % 2 else c.sigma, z)
    if c.name in _SPEC:
        _POLICIES[key] = pol
    return pol


@functools.lru_cache(maxsize=None)
def trajectory(name, member, mask=0b1111, steps=H_TOP, seed=None):
    """gru_oracle.rollout of one member: the source of the CPU conditions."""
    c = case(name, seed)
    s0 = philox_ref.env_init_state(c.seed, ITER, ENVS)
    return G.rollout(policy_for(c, member), c.mu, c.nu, mask, c.A, c.B, s0,
                     steps)


def decided(ro):
    """[steps][E]: the oracle calls the action of step t decided."""
    return np.abs(ro.logits[..., 1] - ro.logits[..., 0]) > ro.tol_l.sum(-1)


def least_share(name, seed=None, members=MEMBERS, horizons=None):
    """Least decided share over the members and the checked h of a set."""
    hs = case(name).horizons if horizons is None else horizons
    return min(float(decided(trajectory(name, m, seed=seed))[list(hs)]
                     .mean(-1).min()) for m in members)


# ---- the comparison ---------------------------------------------------------

def worse(a, b):
    """max(a, b) that a NaN wins from either side: a kernel that returns
    NaN must fail, whichever member it is in."""
    return b if b > a or b != b else a


def compare_member(c, member, mask, h, s0, hid0, s1, hid1, f0, f1):
    """One member of a launch pair: worst error / tolerance of h', of the
    state (either outcome of the env step where the oracle calls the action
    undecided; no env is left out) and of the reward increment, and the
    decided share."""
    pol = policy_for(c, member)
    x, x_slack = G.observe(s0, c.mu, c.nu, mask)
    want_h, want_l, tol_h, tol_l = G.cell(pol, x, hid0, x_slack)
    out = {"h": float((np.abs(hid1.astype(np.float64) - want_h)
                       / tol_h).max())}
    act = want_l[:, 1] > want_l[:, 0]
    close = np.abs(want_l[:, 1] - want_l[:, 0]) <= tol_l.sum(-1)
    sa, tol_s = G.env_step(s0, act, c.A, c.B)
    sb, _ = G.env_step(s0, ~act, c.A, c.B)
    ra = (np.abs(s1 - sa) / tol_s).max(-1)
    rb = (np.abs(s1 - sb) / tol_s).max(-1)
    ratio = np.where(close, np.minimum(ra, rb), ra)
    out["s"] = float(np.nan if np.isnan(ra).any() or np.isnan(rb).any()
                     else ratio.max())
    # The reward of step h from the kernel's own state at h + 1.  Per step
    # 3 roundings of 0.1*s*s and the subtract, then h + 1 adds per thread
    # and 3 + 6 adds across dims and envs, on sums <= mag.
    s64 = s1.astype(np.float64)
    rew = ENVS - G.C01 * (s64 * s64).sum()
    mag = (ENVS + G.C01 * (s64 * s64).sum()) * (h + 1)
    tol_f = (h + 14) * G.U * mag
    out["f"] = float(abs(ENVS * (float(f1) - float(f0)) - rew) / tol_f)
    return out, float(1.0 - close.mean())


def compare_stats(h, pop, s0_all, st0, st1):
    """obs_stat[h + 1] - obs_stat[h] is the states at step h over all
    members: (worst error / tolerance, the count increment is exact).

    Each launch rounds on its own.  A term passes h + 1 adds in its thread,
    6 in the shuffle tree over the envs and 1 + 8 in obs_stat_reduce (pop <=
    256), and a square is rounded once before it enters: h + 17 roundings,
    each within U of a partial sum that never exceeds sum|terms|.  For the
    squares that is the slot itself; for the n = 64 pop (h + 1) plain terms
    it is at most sqrt(n * sumsq).  The shorter launch's bound is no larger,
    hence the 2."""
    s64 = s0_all.astype(np.float64)
    want = np.concatenate([s64.sum((0, 1)), (s64 * s64).sum((0, 1))])
    sumsq = st1[4:8].astype(np.float64)
    big = np.concatenate([np.sqrt(ENVS * pop * (h + 1) * sumsq), sumsq])
    tol_st = 2.0 * (h + 17) * G.U * big
    # a slot that stayed 0 has the tolerance 0: x / 0 is inf and 0 / 0 NaN,
    # and both fail
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float((np.abs(st1[:8].astype(np.float64) - st0[:8] - want)
                       / tol_st).max())
    return ratio, bool(st1[8] - st0[8] == ENVS * pop)


Verdict = collections.namedtuple("Verdict", [
    "worst",       # {"h", "s", "f", "stat"}: worst error / tolerance
    "count_ok",    # the obs count grew by exactly 64 * pop
    "shares"])     # decided share per member


def compare_pair(c, offset, mask, h, run0, run1):
    """The whole one-step check of the launches at horizons h and h + 1 of
    ``pop`` members from ``offset``: every member, env and hidden unit."""
    f0, st0, s0, hid0 = run0
    f1, st1, s1, hid1 = run1
    pop = len(f0)
    worst, shares = {}, []
    for m in range(pop):
        got, share = compare_member(c, offset + m, mask, h, s0[m], hid0[m],
                                    s1[m], hid1[m], f0[m], f1[m])
        for k, v in got.items():
            worst[k] = worse(worst.get(k, 0.0), v)
        shares.append(share)
    worst["stat"], count_ok = compare_stats(h, pop, s0, st0, st1)
    return Verdict(worst, count_ok, shares)


def passes(v):
    return v.count_ok and all(r <= 1.0 for r in v.worst.values())


def policy_step_ratios(theta, x, h, logits, hnew):
    """gru_policy_step's outputs against gru_oracle.cell: worst error /
    tolerance of (h', logits), as test_gru_gpu.py compares them."""
    want_h, want_l, tol_h, tol_l = G.cell(G.make_policy(theta), x, h)
    return (float((np.abs(np.asarray(hnew, np.float64) - want_h)
                   / tol_h).max()),
            float((np.abs(np.asarray(logits, np.float64) - want_l)
                   / tol_l).max()))


# ---- saturation ---------------------------------------------------------------
# fast_sigmoid(a) = rcp(1 + exp2(-a log2e)): exp2 overflows to inf below
# a = -128 / log2e = -88.8, and 1 + exp2(..) is 1 above a = 150 / log2e = 104
# (exp2 itself flushes to 0 there)
PRE_OVERFLOW, PRE_UNDERFLOW = -88.8, 104.0
MID_LO, MID_HI = 0.05, 0.95


def saturation(ro, h):
    """Of the r and z gates of step h: (least pre-activation, largest,
    share of gate values in (0.05, 0.95))."""
    a = ro.pre[h, :2]
    g = 1.0 / (1.0 + np.exp(-a))
    return (float(a.min()), float(a.max()),
            float(((g > MID_LO) & (g < MID_HI)).mean()))


# ---- stand-in kernels -----------------------------------------------------------
DEFECTS = ("no_clamp", "clamp_4", "mask_ignored", "mask_reversed",
           "stats_skip_hidden", "wrong_parity", "h_carried_bf16",
           "sign_not_flipped", "reward_dropped", "reward_old_state")


def _bf16(v):
    return G.bf16_round(v)[0]


def standin_cell(pol, x, h, hb, defect=None):
    """A plain float64 GRU step with the kernel's roundings: (h', logits).
    ``hb`` is the bf16 copy of h that the matmul reads."""
    r = 1.0 / (1.0 + np.exp(-(pol.b[0] + x @ pol.wi[0].T + hb @ pol.wh[0].T)))
    z = 1.0 / (1.0 + np.exp(-(pol.b[1] + x @ pol.wi[1].T + hb @ pol.wh[1].T)))
    n = np.tanh(pol.b[2] + x @ pol.wi[2].T
                + r * (pol.b[3] + hb @ pol.wh[2].T))
    hc = _bf16(h) if defect == "h_carried_bf16" else h
    hn = n + z * (hc - n)
    hl = _bf16(hn) if defect == "logits_from_bf16" else hn
    return hn, hl @ pol.wo.T + pol.bo


@functools.lru_cache(maxsize=None)
def standin_runs(name, mask, defect, top, offset=OFFSET, pop=POP):
    """The runs of a stand-in "kernel" at every horizon 0 .. top: a list of
    ``(fitness, obs_stat, final_state, final_hidden)``.  The defect acts at
    every step, and the stand-in follows its own trajectory."""
    c = case(name)
    mu = c.mu.astype(np.float64)
    rstd = 1.0 / np.sqrt(c.nu.astype(np.float64) + G.C1EM4)
    A, B = c.A.astype(np.float64), c.B.astype(np.float64)
    bits = [(mask >> d) & 1 for d in range(G.OBS)]
    if defect == "mask_ignored":
        bits = [1] * G.OBS
    elif defect == "mask_reversed":
        bits = bits[::-1]
    vis = np.array(bits, dtype=bool)
    counted = np.array([(mask >> d) & 1 for d in range(G.OBS)], bool) \
        if defect == "stats_skip_hidden" else np.ones(G.OBS, bool)
    lim = {"no_clamp": np.inf, "clamp_4": 4.0}.get(defect, 5.0)
    per_member = []
    for member in range(offset, offset + pop):
        z = philox_ref.noise_for_pair(c.seed, ITER, member // 2,
                                      G.GRU_NPARAMS)
        sgn = -c.sigma if member % 2 else c.sigma
        if defect == "sign_not_flipped":
            sgn = c.sigma
        pol = G.make_policy(c.theta, sgn, z)
        s = philox_ref.env_init_state(c.seed, ITER, ENVS).astype(np.float64)
        h = np.zeros((ENVS, G.HID))
        hb_other = np.zeros_like(h)     # the other half of the double buffer
        ret = np.zeros(ENVS)
        stat = np.zeros(2 * G.OBS)
        outs = []
        for t in range(top + 1):
            outs.append((ret.mean(), stat.copy(), s.astype(np.float32),
                         h.astype(np.float32)))
            if t == top:
                break
            stat += np.concatenate([(s * counted).sum(0),
                                    (s * s * counted).sum(0)])
            x = _bf16(np.where(vis, np.clip((s - mu) * rstd, -lim, lim), 0.0))
            hb = _bf16(h)
            hn, logits = standin_cell(
                pol, x, h, hb_other if defect == "wrong_parity" else hb,
                defect)
            hb_other = hb
            asign = np.where(logits[:, 1] > logits[:, 0], 1.0, -1.0)
            snew = (G.C008 * np.tanh(s @ A.T) + G.C097 * s
                    + G.C005 * B * asign[:, None])
            snew = snew.astype(np.float32).astype(np.float64)
            sr = s if defect == "reward_old_state" else snew
            if defect != "reward_dropped":
                ret = ret + 1.0 - G.C01 * (sr * sr).sum(-1)
            s, h = snew, hn.astype(np.float32).astype(np.float64)
        per_member.append(outs)
    runs = []
    for t in range(top + 1):
        stat = sum(per_member[m][t][1] for m in range(pop))
        runs.append((
            np.array([per_member[m][t][0] for m in range(pop)], np.float32),
            np.concatenate([stat, [ENVS * pop * t]]).astype(np.float32),
            np.stack([per_member[m][t][2] for m in range(pop)]),
            np.stack([per_member[m][t][3] for m in range(pop)])))
    return runs


def standin_verdict(name, mask, defect, h, top=None):
    if top is None:
        top = max(case(name).horizons) + 1
    runs = standin_runs(name, mask, defect, top)
    return compare_pair(case(name), OFFSET, mask, h, runs[h], runs[h + 1])
