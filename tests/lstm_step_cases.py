"""One-step-at-a-time checks of the LSTM rollout kernel at depth, under
saturation and under the clamp, shared by tests/test_lstm_step.py (CPU) and
tests/gpu/test_lstm_step_gpu.py.  Everything here runs without a GPU and
nothing here is modified by a test.  It is tests/gru_step_cases.py for the
kernel with two carried states.

The comparison is the restart scheme of tests/gpu/test_lstm_gpu.py: the
kernel's own fp32 ``(state, hidden, cell)`` at horizon h starts ONE step of
``lstm_oracle``, which is compared with the kernel's ``(state, hidden,
cell)`` at h + 1.  Nothing accumulates, so the tolerances of
``lstm_oracle.cell`` and ``env_step`` are used as they are.  A "run" below is
what one launch with ``return_final=True`` returns, as numpy arrays:
``(fitness[pop], obs_stat[9], final_state[pop][64][4],
final_hidden[pop][64][64], final_cell[pop][64][64])``.  The GPU tests feed
``compare_pair`` with the kernel's runs, the CPU tests with the runs of a
plain float64 stand-in that carries one defect at a time.  Derivations and
figures: profiles/lstm.md, "One step at a time, at depth".
"""

import collections
import functools

import numpy as np

from fiber_amd.es import lstm_oracle as L
from fiber_amd.es import philox_ref
from fiber_amd.es.rollout_oracle import C005, C008, C097, C1EM4

ENVS = 64
WORLD_SEED, ITER = 4321, 3      # the ``world`` of tests/gpu/test_lstm_gpu.py
OFFSET, POP = 2, 4              # members 2, 3, 4, 5: two whole pairs
MEMBERS = tuple(range(OFFSET, OFFSET + POP))
CAP = 0.90                      # least decided share per (member, h)

# horizons h of the (h, h + 1) launch pairs: both parities of the h double
# buffer (and so both of "the last step wrote hfin"), and 199, whose h + 1 is
# the engine's default horizon
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
    # lstm_policy_step takes theta as it is, so the bit-for-bit comparison
    # with the serving kernel needs sigma 0: "saturated" without the noise,
    # as "base0" is "base" without it.  Not one of the SETS.
    "saturated0": (8.0, 0.0, False, H_SERVING[-1:]),
}
SETS = ("base0", "base", "wide", "saturated", "clamp")
# (set, h) of the comparison with the serving kernel
SERVING = tuple(("base0", h) for h in H_SERVING) + (
    ("saturated0", H_SERVING[-1]),)

# The launch seed (noise and env init states) of a set is the first of
# WORLD_SEED, WORLD_SEED + 1, .. at which lstm_oracle.rollout leaves at least
# CAP of every member's 64 envs decided at every checked h.  Seeds before it
# are listed as (seed, least share), with the share that ruled them out;
# tests/test_lstm_step.py asserts both.  4321 meets the cap on every set
# (least shares in profiles/lstm.md), so none was rejected.
SEEDS = {name: WORLD_SEED for name in _SPEC}
SEEDS_REJECTED = {name: () for name in _SPEC}

# one launch of 2 members far from pair 0 (pair = member >> 1 = 16383)
FAR_OFFSET, FAR_POP, FAR_H = 32766, 2, 8


@functools.lru_cache(maxsize=None)
def world():
    """theta, mu, nu, env_A, env_B of test_lstm_gpu.py's ``world``, numpy."""
    from fiber_amd.es import init_theta_lstm
    from fiber_amd.es.engine import make_env_params

    A, B = (t.numpy() for t in make_env_params(WORLD_SEED, "cpu"))
    mu = np.array([0.05, -0.1, 0.02, 0.0], dtype=np.float32)
    nu = np.array([0.3, 0.5, 0.2, 0.4], dtype=np.float32)
    out = (init_theta_lstm(WORLD_SEED, "cpu").numpy(), mu, nu, A, B)
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
    z = philox_ref.noise_for_pair(c.seed, ITER, member // 2, L.LSTM_NPARAMS)
    pol = L.make_policy(c.theta, -c.sigma if member % 2 else c.sigma, z)
    if c.name in _SPEC:
        _POLICIES[key] = pol
    return pol


@functools.lru_cache(maxsize=None)
def trajectory(name, member, mask=0b1111, steps=H_TOP, seed=None):
    """lstm_oracle.rollout of one member: the source of the CPU conditions."""
    c = case(name, seed)
    s0 = philox_ref.env_init_state(c.seed, ITER, ENVS)
    return L.rollout(policy_for(c, member), c.mu, c.nu, mask, c.A, c.B, s0,
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


def _ratio(got, want, tol):
    # a zero tolerance divides to inf or NaN, and both fail
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(got.astype(np.float64) - want) / tol
    return float(np.nan if np.isnan(r).any() else r.max())


def compare_member(c, member, mask, h, s0, hid0, cel0, s1, hid1, cel1, f0,
                   f1):
    """One member of a launch pair: worst error / tolerance of h', of c', of
    the state (either outcome of the env step where the oracle calls the
    action undecided; no env is left out) and of the reward increment, and
    the decided share."""
    pol = policy_for(c, member)
    x, x_slack = L.observe(s0, c.mu, c.nu, mask)
    want_h, want_c, want_l, tol_h, tol_c, tol_l = L.cell(pol, x, hid0, cel0,
                                                         x_slack)
    out = {"h": _ratio(hid1, want_h, tol_h), "c": _ratio(cel1, want_c, tol_c)}
    act = want_l[:, 1] > want_l[:, 0]
    close = np.abs(want_l[:, 1] - want_l[:, 0]) <= tol_l.sum(-1)
    sa, tol_s = L.env_step(s0, act, c.A, c.B)
    sb, _ = L.env_step(s0, ~act, c.A, c.B)
    ra = (np.abs(s1 - sa) / tol_s).max(-1)
    rb = (np.abs(s1 - sb) / tol_s).max(-1)
    ratio = np.where(close, np.minimum(ra, rb), ra)
    out["s"] = float(np.nan if np.isnan(ra).any() or np.isnan(rb).any()
                     else ratio.max())
    # The reward of step h from the kernel's own state at h + 1.  Per step
    # 3 roundings of 0.1*s*s and the subtract, then h + 1 adds per thread
    # and 3 + 6 adds across dims and envs, on sums <= mag.
    s64 = s1.astype(np.float64)
    rew = ENVS - L.C01 * (s64 * s64).sum()
    mag = (ENVS + L.C01 * (s64 * s64).sum()) * (h + 1)
    tol_f = (h + 14) * L.U * mag
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
    tol_st = 2.0 * (h + 17) * L.U * big
    # a slot that stayed 0 has the tolerance 0: x / 0 is inf and 0 / 0 NaN,
    # and both fail
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float((np.abs(st1[:8].astype(np.float64) - st0[:8] - want)
                       / tol_st).max())
    return ratio, bool(st1[8] - st0[8] == ENVS * pop)


Verdict = collections.namedtuple("Verdict", [
    "worst",       # {"h", "c", "s", "f", "stat"}: worst error / tolerance
    "count_ok",    # the obs count grew by exactly 64 * pop
    "shares"])     # decided share per member


def compare_pair(c, offset, mask, h, run0, run1):
    """The whole one-step check of the launches at horizons h and h + 1 of
    ``pop`` members from ``offset``: every member, env and hidden unit."""
    f0, st0, s0, hid0, cel0 = run0
    f1, st1, s1, hid1, cel1 = run1
    pop = len(f0)
    worst, shares = {}, []
    for m in range(pop):
        got, share = compare_member(c, offset + m, mask, h, s0[m], hid0[m],
                                    cel0[m], s1[m], hid1[m], cel1[m], f0[m],
                                    f1[m])
        for k, v in got.items():
            worst[k] = worse(worst.get(k, 0.0), v)
        shares.append(share)
    worst["stat"], count_ok = compare_stats(h, pop, s0, st0, st1)
    return Verdict(worst, count_ok, shares)


def passes(v):
    return v.count_ok and all(r <= 1.0 for r in v.worst.values())


def policy_step_ratios(theta, x, h, c, logits, hnew, cnew):
    """lstm_policy_step's outputs against lstm_oracle.cell: worst error /
    tolerance of (h', c', logits), as test_lstm_gpu.py compares them."""
    want_h, want_c, want_l, tol_h, tol_c, tol_l = L.cell(
        L.make_policy(theta), x, h, c)
    return (_ratio(np.asarray(hnew), want_h, tol_h),
            _ratio(np.asarray(cnew), want_c, tol_c),
            _ratio(np.asarray(logits), want_l, tol_l))


# ---- saturation ---------------------------------------------------------------
# fast_sigmoid(a) = rcp(1 + exp2(-a log2e)): exp2 overflows to inf below
# a = -128 / log2e = -88.8, and 1 + exp2(..) is 1 above a = 150 / log2e = 104
# (exp2 itself flushes to 0 there)
PRE_OVERFLOW, PRE_UNDERFLOW = -88.8, 104.0
MID_LO, MID_HI = 0.05, 0.95
SIGMOID_GATES = (0, 1, 3)       # i, f, o of (i, f, g, o)


def saturation(ro, h):
    """Of the i, f and o gates of step h: (least pre-activation, largest,
    share of gate values in (0.05, 0.95))."""
    a = ro.pre[h][list(SIGMOID_GATES)]
    g = 1.0 / (1.0 + np.exp(-a))
    return (float(a.min()), float(a.max()),
            float(((g > MID_LO) & (g < MID_HI)).mean()))


# ---- stand-in kernels -----------------------------------------------------------
# The ten of gru_step_cases.py.  "h_carried_bf16" reads here as: the fp32 h'
# that the kernel keeps (what the logits read and what final_hidden returns)
# is rounded to bf16; the matmul reads bf16(h) in the sound kernel too.
GRU_DEFECTS = ("no_clamp", "clamp_4", "mask_ignored", "mask_reversed",
               "stats_skip_hidden", "wrong_parity", "h_carried_bf16",
               "sign_not_flipped", "reward_dropped", "reward_old_state")
# and those only a kernel with a cell state can have
LSTM_DEFECTS = ("c_carried_bf16", "c_tiles_swapped", "hfin_stale",
                "cell_stale", "hfin_not_zeroed", "gates_fo_swapped")
DEFECTS = GRU_DEFECTS + LSTM_DEFECTS

# env e <-> e + 16 within each half of the block: the two column tiles whose
# cell states one lane holds in c[2]
TILE_SWAP = np.arange(ENVS) ^ 16
HFIN_GARBAGE = 0.25             # "hfin_not_zeroed": what the tile held


def _bf16(v):
    return L.bf16_round(v)[0]


def _f32(v):
    return v.astype(np.float32).astype(np.float64)


def standin_cell(pol, x, c, hb, defect=None):
    """A plain float64 LSTM step with the kernel's roundings: (h', c',
    logits).  ``hb`` is the bf16 copy of h that the matmul reads; the carried
    fp32 h itself enters nowhere else."""
    ig, fg, gg, og = (pol.b[g] + x @ pol.wi[g].T + hb @ pol.wh[g].T
                      for g in range(L.GATES))
    ig, fg, og = (1.0 / (1.0 + np.exp(-a)) for a in (ig, fg, og))
    gg = np.tanh(gg)
    if defect == "gates_fo_swapped":
        fg, og = og, fg
    cc = _bf16(c) if defect == "c_carried_bf16" else c
    cn = _f32(fg * cc + ig * gg)
    hn = _f32(og * np.tanh(cn))
    if defect == "h_carried_bf16":
        hn = _bf16(hn)
    return hn, cn, hn @ pol.wo.T + pol.bo


@functools.lru_cache(maxsize=None)
def standin_runs(name, mask, defect, top, keep=None, offset=OFFSET, pop=POP):
    """The runs of a stand-in "kernel" at the horizons ``keep`` (all of
    0 .. top if None): ``{horizon: (fitness, obs_stat, final_state,
    final_hidden, final_cell)}``.  The defect acts at every step, and the
    stand-in follows its own trajectory."""
    c = case(name)
    keep = set(range(top + 1)) if keep is None else set(keep)
    mu = c.mu.astype(np.float64)
    rstd = 1.0 / np.sqrt(c.nu.astype(np.float64) + C1EM4)
    A, B = c.A.astype(np.float64), c.B.astype(np.float64)
    bits = [(mask >> d) & 1 for d in range(L.OBS)]
    if defect == "mask_ignored":
        bits = [1] * L.OBS
    elif defect == "mask_reversed":
        bits = bits[::-1]
    vis = np.array(bits, dtype=bool)
    counted = np.array([(mask >> d) & 1 for d in range(L.OBS)], bool) \
        if defect == "stats_skip_hidden" else np.ones(L.OBS, bool)
    lim = {"no_clamp": np.inf, "clamp_4": 4.0}.get(defect, 5.0)
    per_member = []
    for member in range(offset, offset + pop):
        z = philox_ref.noise_for_pair(c.seed, ITER, member // 2,
                                      L.LSTM_NPARAMS)
        sgn = -c.sigma if member % 2 else c.sigma
        if defect == "sign_not_flipped":
            sgn = c.sigma
        pol = L.make_policy(c.theta, sgn, z)
        s = philox_ref.env_init_state(c.seed, ITER, ENVS).astype(np.float64)
        h = np.zeros((ENVS, L.HID))
        cel = np.zeros((ENVS, L.HID))
        h_before = np.full_like(
            h, HFIN_GARBAGE if defect == "hfin_not_zeroed" else 0.0)
        c_before = np.zeros_like(cel)
        hb_other = np.zeros_like(h)     # the other half of the double buffer
        ret = np.zeros(ENVS)
        stat = np.zeros(2 * L.OBS)
        outs = {}
        for t in range(top + 1):
            if t in keep:
                h_out = h_before if defect == "hfin_stale" or (
                    defect == "hfin_not_zeroed" and t == 0) else h
                c_out = c_before if defect == "cell_stale" else cel
                outs[t] = (ret.mean(), stat.copy(), s.astype(np.float32),
                           h_out.astype(np.float32),
                           c_out.astype(np.float32))
            if t == top:
                break
            stat += np.concatenate([(s * counted).sum(0),
                                    (s * s * counted).sum(0)])
            x = _bf16(np.where(vis, np.clip((s - mu) * rstd, -lim, lim), 0.0))
            hb = _bf16(h)
            hn, cn, logits = standin_cell(
                pol, x, cel, hb_other if defect == "wrong_parity" else hb,
                defect)
            if defect == "c_tiles_swapped":
                cn = cn[TILE_SWAP]
            hb_other = hb
            asign = np.where(logits[:, 1] > logits[:, 0], 1.0, -1.0)
            snew = _f32(C008 * np.tanh(s @ A.T) + C097 * s
                        + C005 * B * asign[:, None])
            sr = s if defect == "reward_old_state" else snew
            if defect != "reward_dropped":
                ret = ret + 1.0 - L.C01 * (sr * sr).sum(-1)
            h_before, c_before = h, cel
            s, h, cel = snew, hn, cn
        per_member.append(outs)
    runs = {}
    for t in sorted(keep):
        stat = sum(per_member[m][t][1] for m in range(pop))
        runs[t] = (
            np.array([per_member[m][t][0] for m in range(pop)], np.float32),
            np.concatenate([stat, [ENVS * pop * t]]).astype(np.float32),
            np.stack([per_member[m][t][2] for m in range(pop)]),
            np.stack([per_member[m][t][3] for m in range(pop)]),
            np.stack([per_member[m][t][4] for m in range(pop)]))
    return runs


def standin_horizons(name):
    """The launches that the checked h of a set need: h and h + 1."""
    return tuple(sorted({t for h in case(name).horizons for t in (h, h + 1)}))


def standin_verdict(name, mask, defect, h, top=None):
    if top is None:
        runs = standin_runs(name, mask, defect,
                            max(case(name).horizons) + 1,
                            standin_horizons(name))
    else:
        runs = standin_runs(name, mask, defect, top)
    return compare_pair(case(name), OFFSET, mask, h, runs[h], runs[h + 1])
