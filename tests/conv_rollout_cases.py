"""Teacher-forced check of ONE step of ``ConvESEngine.rollout``, the cases
the CPU and GPU rollout-chain tests share, and an fp32 emulation of
``_rollout_body`` (CPU only).

After ``rollout(it)`` at horizon h an engine's buffers hold the noise and
activations of its last step (t = h-1) and the state / racc after h steps;
an engine of horizon h-1 holds what went INTO that step.  ``check_step``
takes the two buffer sets as dicts of CPU tensors and checks step h layer
by layer, each layer fed with the device's own inputs, against the fp64
references of ``fiber_amd.es.conv_reference``.  Every tolerance is derived
next to its use or in conv_reference.py / update_oracle.py; none is fitted
to what a kernel returns.

Stages, in the order they are checked (``StageError.stage``):

  precondition  env_B makes a wrong action visible; few undecided envs
  noise         znoise[c] of every chunk = numpy Philox mirror (seed, it, t)
  init          t = 0 only: state_0 = 0.3 * z64 of conv_env_init, racc_0 = 0
  layer1        act1 against obs(znoise[c], state_{h-1}) (x) w1_fp8
  layer2        act2 against the device's act1
  fc            act3 against the device's act2
  head          state_h, racc_h against the env step for the argmax action
  fitness       returned fitness = mean of the device's racc rows
  wpert         wpert[m] = theta +- sigma * z64 of pair (rank*pop + m) // 2
"""

import functools

import numpy as np
import torch

from fiber_amd.es import conv_reference as cr
from fiber_amd.es import philox_ref
from fiber_amd.es import update_oracle as uo
from fiber_amd.es.rollout_oracle import ULP, Z_SIDE_ULPS

E = cr.CENV
NOISE_BYTES = E * cr.IMG * cr.IMG * 4
TAG_OBS = np.uint32(0x45530003)
# conv_head_env's state / racc against fp64: a handful of fp32 roundings of
# values below 4 plus 0.08 * TAU (tests/gpu/test_conv_layers.py TestHeadEnv)
TOL = 2.0 ** -18
# racc.mean(dim=1): 15 fp32 adds of partial sums below 16 * 4 = 64, each
# within 2^-24 * 64 = 2^-18; the division by 16 is exact, so the mean is
# within 15/16 * 2^-18
FIT_TOL = 2.0 ** -18
SIGMA = 0.02
BLOCK_MEMBERS = 4      # fp64 patch tensors stay at <= 64 envs

STAGES = ("precondition", "noise", "init", "layer1", "layer2", "fc", "head",
          "fitness", "wpert")

# seed: chosen by ``search_seed`` (CPU, fp32 emulation): the first seed from
# 1 at which every env of every checked step has a top-two logit gap above
# 4x its largest logit bound and the actions take >= 4 distinct values.
CASES = {
    "two_chunks": dict(pop=8, chunks=2, horizons=(1, 2, 3), capture=0,
                       iteration=3, rank=0, world=1, seed=1),
    "eight_chunks": dict(pop=32, chunks=8, horizons=(1, 2), capture=None,
                         iteration=2, rank=0, world=1, seed=6),
    "single_eager": dict(pop=2, chunks=1, horizons=(1,), capture=None,
                         iteration=1, rank=0, world=1, seed=1),
    "second_shard": dict(pop=4, chunks=1, horizons=(1,), capture=None,
                         iteration=1, rank=1, world=2, seed=1),
}


class StageError(AssertionError):
    def __init__(self, stage, msg):
        super().__init__("[%s] %s" % (stage, msg))
        self.stage = stage


# ---------------------------------------------------------------------------
# references the step check adds to conv_reference.py
# ---------------------------------------------------------------------------


@functools.lru_cache(maxsize=16)
def noise_mirror(seed, iteration, t):
    """conv_noisegen's bytes [16][84*84*4]: integer -> float32 conversion
    and one float32 product, exact in numpy, so the e4m3 bytes are too."""
    p = np.arange(cr.IMG * cr.IMG, dtype=np.uint32)
    rows = []
    for e in range(E):
        z = philox_ref.uniform4(seed, iteration,
                                np.uint32(e) * np.ones_like(p), p, TAG_OBS,
                                np.uint32(t))
        rows.append(cr.e4m3_bytes(torch.from_numpy(
            (np.float32(0.52) * z).astype(np.float32))).reshape(-1))
    return torch.stack(rows)


def init_state_fp64(seed, iteration):
    """conv_env_init's state [16][4] in fp64, and its tolerance: z within
    Z_SIDE_ULPS ulp of the fp64 Box-Muller of the same fp32 arguments
    (rollout_oracle.py), one more ulp for the product by 0.3f."""
    e = np.arange(E, dtype=np.uint32)
    z = uo.normals_fp64(np.uint32(seed), np.uint32(iteration), e,
                        np.uint32(0), philox_ref.TAG_ENV)
    want = float(np.float32(0.3)) * z
    return (torch.from_numpy(want),
            torch.from_numpy((Z_SIDE_ULPS + 1) * ULP * np.abs(want)))


@functools.lru_cache(maxsize=40)
def _pair_noise64(seed, iteration, pair):
    return torch.from_numpy(uo.noise_fp64(seed, iteration, pair, cr.NP_CONV))


def wpert_reference(theta, sigma, seed, iteration, pair, sign):
    """(want64, half_ulp, slack) of one member's wpert[:NP_CONV].

    es_perturb computes bf16(theta + sigma * z) in fp32, sigma passed as a
    float.  Against want = theta +- sigma32 * z64:
      * the device's z is within Z_SIDE_ULPS fp32 ulp of z64 (update_oracle:
        same fp32 arguments, logf / sinf / cosf within 2 ulp), and the
        product sigma * z rounds once: sigma * (Z_SIDE_ULPS + 1) ulp of z;
      * the sum (or the fma it contracts to) rounds once: one ulp of want;
      * the rounding to bf16 adds half a bf16 ulp at the slack-widened
        magnitude."""
    z = _pair_noise64(int(seed), int(iteration), int(pair))
    s32 = float(np.float32(sigma))
    want = theta.double() + sign * s32 * z
    slack = s32 * (Z_SIDE_ULPS + 1) * ULP * z.abs() + ULP * want.abs()
    return want, 0.5 * cr.ulp_bf16(want.abs() + slack), slack


def check_perturbation(cur, theta, sigma, seed, iteration, rank, pop_per_gpu,
                       members, pairs_total=None):
    """Stage ``wpert`` for the listed local members.  Returns (worst
    (err - 1/2 ulp) / slack, smallest fraction of coordinates on which the
    neighbouring pair misses the tolerance)."""
    worst, miss_min = -np.inf, 1.0
    for m in members:
        g = rank * pop_per_gpu + m
        pair, sign = g // 2, (-1.0 if g % 2 else 1.0)
        got = cur["wpert"][m, :cr.NP_CONV].double()
        want, half_ulp, slack = wpert_reference(theta, sigma, seed,
                                                iteration, pair, sign)
        err = (got - want).abs()
        bad = ~(err <= half_ulp + slack)
        if bool(bad.any()):
            hint = ""
            for p in range(pairs_total or (pop_per_gpu * (rank + 1)) // 2):
                for sg in (1.0, -1.0):
                    w2, h2, s2 = wpert_reference(theta, sigma, seed,
                                                 iteration, p, sg)
                    if bool(((got - w2).abs() <= h2 + s2).all()):
                        hint = "; it IS pair %d sign %+d" % (p, sg)
            j = int(torch.argmax(err - half_ulp - slack))
            raise StageError("wpert", (
                "member %d (global %d) is not theta %s sigma*z of pair %d: "
                "%d of %d coordinates outside the tolerance, worst j=%d got "
                "%.9g want %.9g allowed %.3g%s") % (
                    m, g, "+" if sign > 0 else "-", pair, int(bad.sum()),
                    bad.numel(), j, got[j], want[j],
                    (half_ulp + slack)[j], hint))
        worst = max(worst, float(((err - half_ulp) / slack).max()))
        # the tolerance names the pair: the next pair's vector misses it
        w2, _, _ = wpert_reference(theta, sigma, seed, iteration, pair + 1,
                                   sign)
        miss = float(((got - w2).abs() > half_ulp + slack).double().mean())
        if not miss > 0.99:
            raise StageError("wpert", "pair %d's vector fits member %d on "
                             "%.2f%% of coordinates: the check cannot name "
                             "the pair" % (pair + 1, m, 100 * (1 - miss)))
        miss_min = min(miss_min, miss)
        # the two fp8 copies are roundings of the same fp32 value
        # (test_sigma_nonzero_roundings_agree)
        bfv = got
        for name, f8, b in (
                ("w3_fp8", cur["w3_fp8"][m], bfv[cr.OFF_W3:cr.OFF_B3]),
                ("w1_fp8", cur["w1_fp8"][m], bfv[:cr.OFF_B1])):
            d = (cr.e4m3_val(f8) - b).abs()
            badf = ~(d <= 0.5 * cr.ulp_e4m3(b) + 0.5 * cr.ulp_bf16(b))
            if bool(badf.any()):
                j = int(torch.nonzero(badf)[0])
                raise StageError("wpert", (
                    "member %d %s[%d] = %.9g is not a rounding of the value "
                    "wpert holds as %.9g (%d of %d differ)") % (
                        m, name, j, cr.e4m3_val(f8)[j], b[j],
                        int(badf.sum()), badf.numel()))
    return worst, miss_min


# ---------------------------------------------------------------------------
# the step check
# ---------------------------------------------------------------------------


def head_decisions(act3, w4, b4):
    """Per env: logits, bound, first maximum, ``decided`` and the candidate
    mask [E][6].

    Decided: the top-two logit gap exceeds the sum of those two logits'
    bounds; the only candidate is the first maximum.  Undecided: every
    action whose logit lies within (its bound + the maximum's bound) of the
    maximum is a candidate, except an action whose W4 row and bias are
    bit-identical to an EARLIER action's: the kernel computes the same fp32
    value for both and its strict ``>`` keeps the earlier one."""
    nenv = act3.shape[0]
    m = nenv // E
    zero = torch.zeros(nenv, 4)
    logits, a1, _, _, bound = cr.head_env_reference(
        act3, w4, b4, zero, torch.zeros(4, 4), torch.zeros(4),
        torch.zeros(nenv))
    idx = torch.arange(nenv)
    l1, bd1 = logits[idx, a1], bound[idx, a1]
    rest = logits.clone()
    rest[idx, a1] = -np.inf
    a2 = rest.argmax(dim=1)
    gap = l1 - logits[idx, a2]
    decided = gap > bd1 + bound[idx, a2]
    near = (l1[:, None] - logits) <= (bound + bd1[:, None])
    w = w4.reshape(m, 6, 256).view(torch.int16)
    b = b4.reshape(m, 6).contiguous().view(torch.int16)
    shadow = torch.zeros(m, 6, dtype=torch.bool)
    for a in range(1, 6):
        for a0 in range(a):
            shadow[:, a] |= (w[:, a] == w[:, a0]).all(dim=1) & \
                (b[:, a] == b[:, a0])
    first = torch.nn.functional.one_hot(a1, 6).bool()
    cand = torch.where(decided[:, None], first,
                       (near & ~shadow.repeat_interleave(E, dim=0)) | first)
    ratio = gap / bound.max(dim=1).values
    return dict(logits=logits, bound=bound, action=a1, decided=decided,
                cand=cand, gap_over_bound=ratio)


def check_head(state_prev, racc_prev, state_cur, racc_cur, hd, env_A, env_B,
               t):
    """Stage ``head``: for a decided env, state and racc must be within TOL
    of the fp64 env step for the first maximum; for an undecided env, of
    the env step for ONE of its candidate actions (``head_decisions``).
    No env is exempt."""
    nenv = hd["logits"].shape[0]
    rep = {}
    # a reward is at most 1, so racc after t steps is at most t; TOL's
    # derivation needs racc < 4
    racc_prev = racc_prev.reshape(-1)
    if not bool((racc_prev.double() <= t + TOL).all()):
        be = int(torch.argmax(racc_prev))
        raise StageError("head", (
            "racc_%d of member %d env %d is %.9g: more than %d rewards of at "
            "most 1") % (t, be // E, be % E, racc_prev[be], t))
    st_got = state_cur.double().reshape(nenv, 4)
    ra_got = racc_cur.double().reshape(-1)
    best = torch.full((nenv,), np.inf, dtype=torch.float64)
    best_any = best.clone()
    chosen = torch.full((nenv,), -1, dtype=torch.long)
    chosen_any = chosen.clone()
    es_at = torch.zeros(nenv, dtype=torch.float64)
    er_at = torch.zeros(nenv, dtype=torch.float64)
    for act in range(6):
        snew, rnew = cr.env_step_reference(
            state_prev, torch.full((nenv,), act), env_A, env_B, racc_prev)
        es = (st_got - snew).abs().max(dim=1).values
        er = (ra_got - rnew).abs()
        err = torch.nan_to_num(torch.maximum(es, er), nan=np.inf)
        better = err < best_any
        best_any = torch.where(better, err, best_any)
        chosen_any = torch.where(better, torch.full_like(chosen, act),
                                 chosen_any)
        err_c = torch.where(hd["cand"][:, act], err,
                            torch.full_like(err, np.inf))
        better = err_c < best
        best = torch.where(better, err_c, best)
        chosen = torch.where(better, torch.full_like(chosen, act), chosen)
        es_at = torch.where(better, es, es_at)
        er_at = torch.where(better, er, er_at)
    bad = ~(best <= TOL)
    if bool(bad.any()):
        be = int(torch.nonzero(bad)[0])
        cands = torch.nonzero(hd["cand"][be]).reshape(-1).tolist()
        raise StageError("head", (
            "%d of %d envs; first: member %d env %d (%s, logits %s, "
            "candidate actions %s): state_%d / racc_%d are %.3g away from "
            "the env step for any candidate (tolerance %.3g); the closest "
            "action is %d at %.3g; state %s racc %.9g, state_%d %s racc_%d "
            "%.9g") % (
                int(bad.sum()), nenv, be // E, be % E,
                "decided" if bool(hd["decided"][be]) else "undecided",
                ["%.6f" % x for x in hd["logits"][be].tolist()], cands,
                t + 1, t + 1, best[be], TOL, int(chosen_any[be]),
                best_any[be], state_cur.reshape(nenv, 4)[be].tolist(),
                ra_got[be], t, state_prev.reshape(nenv, 4)[be].tolist(),
                t, racc_prev[be]))
    rep["state_err_over_tol"] = float(es_at.max()) / TOL
    rep["racc_err_over_tol"] = float(er_at.max()) / TOL
    rep["taken"] = chosen
    return rep


def _bf(t):
    return t if t.dtype == torch.bfloat16 else t.view(torch.bfloat16)


def _layer(got, pre, absdot, K, fmt, bias):
    err, half_ulp, slack = cr.layer_errors(got, pre, absdot, K, fmt, bias)
    ok = ~(err > half_ulp + slack) & torch.isfinite(err)
    return ok, (err - half_ulp) / slack


def _raise_layer(stage, got, pre, absdot, K, fmt, bias, a, b, chunk, extra=""):
    try:
        cr.check_layer(got, pre, absdot, K, fmt, bias, what=stage)
    except AssertionError as exc:
        raise StageError(stage, (
            "chunk %d, members %d..%d (the member index below counts from "
            "member %d)%s\n%s") % (chunk, a, b - 1, a, extra, exc)) from None
    raise StageError(stage, "chunk %d members %d..%d" % (chunk, a, b - 1))


def check_step(prev, cur, const, max_undecided=2, perturb_members=None):
    """Check step ``t = const["t"]`` (the h-th, h = t + 1).

    prev   state [pop*16][4] fp32, racc [pop][16] fp32 after t steps
    cur    znoise [chunks][16*84*84*4] u8, act1/act2/act3, state, racc after
           t + 1 steps, wpert, w1_fp8, w3_fp8, fitness [pop]
    const  seed, iteration, t, chunks, gtab_bf, env_A, env_B; for the wpert
           stage also theta, sigma, rank, pop_per_gpu (and world)

    Returns the worst (err - 1/2 ulp) / slack per layer, the decided /
    undecided counts, the actions taken by decided envs, the smallest
    gap / bound, and the worst state, racc and fitness error over their
    tolerances.  Raises StageError naming (member, env, ...)."""
    seed, it, t = const["seed"], const["iteration"], const["t"]
    chunks = const["chunks"]
    pop = cur["racc"].shape[0]
    nenv = pop * E
    assert pop % chunks == 0
    per = pop // chunks
    env_A, env_B = const["env_A"].cpu(), const["env_B"].cpu()
    gtab = const["gtab_bf"].cpu()
    v = cr.policy_views({"wpert": _bf(cur["wpert"])})
    act1, act3 = _bf(cur["act1"]), _bf(cur["act3"])
    rep = {}

    # -- precondition ------------------------------------------------------
    # the six forces must be distinguishable in the state update
    if not float((0.02 * env_B.abs()).max()) > 100 * TOL:
        raise StageError("precondition", "env_B too small: a wrong action "
                         "would not show in the state")
    hd = head_decisions(act3, v["w4"], v["b4"])
    rep["decided"] = int(hd["decided"].sum())
    rep["undecided"] = nenv - rep["decided"]
    rep["actions"] = sorted(set(hd["action"][hd["decided"]].tolist()))
    rep["min_gap_over_bound"] = float(hd["gap_over_bound"].min())
    if max_undecided is not None and rep["undecided"] > max_undecided:
        raise StageError("precondition", "%d of %d envs undecided (at most "
                         "%d allowed)" % (rep["undecided"], nenv,
                                          max_undecided))

    # -- noise ---------------------------------------------------------------
    want = noise_mirror(seed, it, t).reshape(-1)
    for c in range(chunks):
        got = cur["znoise"][c].reshape(-1)
        if not torch.equal(got, want):
            hint = ""
            for name, (i2, t2) in (("t-1", (it, t - 1)), ("t+1", (it, t + 1)),
                                   ("the capture iteration",
                                    (const.get("capture"), t))):
                if i2 is None or t2 < 0:
                    continue
                if torch.equal(got, noise_mirror(seed, i2, t2).reshape(-1)):
                    hint = "; it IS the noise of %s" % name
            j = int(torch.nonzero(got != want)[0])
            raise StageError("noise", (
                "znoise[%d] is not the noise of (seed %d, iteration %d, "
                "t %d): %d of %d bytes differ, first at env %d offset %d%s")
                % (c, seed, it, t, int((got != want).sum()), got.numel(),
                   j // (NOISE_BYTES // E), j % (NOISE_BYTES // E), hint))

    # -- init ----------------------------------------------------------------
    if t == 0:
        s0, s0_tol = init_state_fp64(seed, it)
        d = (prev["state"].double().reshape(pop, E, 4) - s0[None]).abs()
        bad = ~(d <= s0_tol[None])
        if bool(bad.any()):
            m, e, k = torch.nonzero(bad)[0].tolist()
            raise StageError("init", (
                "state_0 of member %d env %d dim %d is %.9g, conv_env_init "
                "of iteration %d gives %.9g") % (
                    m, e, k, prev["state"].reshape(pop, E, 4)[m, e, k], it,
                    s0[e, k]))
        if bool((prev["racc"] != 0).any()):
            m, e = torch.nonzero(prev["racc"] != 0)[0].tolist()
            raise StageError("init", "racc_0 of member %d env %d is %.9g, "
                             "not 0" % (m, e, prev["racc"][m, e]))
        rep["init_margin"] = float((d / s0_tol[None]).max())

    # -- layers, chunk by chunk, <= 64 envs at a time ------------------------
    margins = {"layer1": -np.inf, "layer2": -np.inf, "fc": -np.inf}
    rep["fused_envs"] = rep["unfused_envs"] = 0
    rep["ambiguous_pixels"] = 0
    for c in range(chunks):
        for a in range(c * per, (c + 1) * per, BLOCK_MEMBERS):
            b = min(a + BLOCK_MEMBERS, (c + 1) * per)
            n = (b - a) * E
            rows = slice(a * E, b * E)
            per_env = lambda x: x[a:b].repeat_interleave(E, dim=0)  # noqa
            zn, st = cur["znoise"][c], prev["state"][rows]

            # layer 1.  ``noise + s * g`` may or may not be contracted to an
            # fma (conv_reference.obs_reference); an env is one workgroup of
            # one compiled kernel, so all of its elements must pass under
            # the same one of the two evaluations.
            obs = cr.obs_reference(zn, st, gtab)
            obs_f = cr.obs_reference(zn, st, gtab, fused=True)
            differ = (obs != obs_f).reshape(n, -1)
            rep["ambiguous_pixels"] += int(differ.sum())
            bias = per_env(v["b1"])[:, None, :]
            got = act1[rows].reshape(n, 400, 16)
            pre, absdot = cr.layer1_reference(obs, cur["w1_fp8"][a:b],
                                              v["b1"][a:b])
            ok, mg = _layer(got, pre, absdot, cr.K_LAYER1, "bf16", bias)
            ok_env = ok.reshape(n, -1).all(dim=1)
            mg_env = mg.reshape(n, -1).max(dim=1).values
            if bool(differ.any()):
                pre_f, absdot_f = cr.layer1_reference(
                    obs_f, cur["w1_fp8"][a:b], v["b1"][a:b])
                ok_f, mg_f = _layer(got, pre_f, absdot_f, cr.K_LAYER1,
                                    "bf16", bias)
                ok_f_env = ok_f.reshape(n, -1).all(dim=1)
                mg_f_env = mg_f.reshape(n, -1).max(dim=1).values
                # reported: the evaluation that explains the env better
                rep["fused_envs"] += int((mg_f_env < mg_env).sum())
                rep["unfused_envs"] += int((mg_f_env > mg_env).sum())
                mg_env = torch.minimum(mg_env, mg_f_env)
                ok_env = ok_env | ok_f_env
            if not bool(ok_env.all()):
                _raise_layer("layer1", got, pre, absdot, cr.K_LAYER1, "bf16",
                             bias, a, b, c, "; %d obs pixels of this block "
                             "depend on fma contraction, neither evaluation "
                             "passes" % int(differ.sum()))
            margins["layer1"] = max(margins["layer1"], float(mg_env.max()))

            # layer 2, from the device's act1
            bias = per_env(v["b2"])[:, None, :]
            got = cur["act2"][rows].reshape(n, 81, 32)
            pre, absdot = cr.layer2_reference(act1[rows], v["w2"][a:b],
                                              v["b2"][a:b])
            ok, mg = _layer(got, pre, absdot, cr.K_LAYER2, "e4m3", bias)
            if not bool(ok.all()):
                _raise_layer("layer2", got, pre, absdot, cr.K_LAYER2, "e4m3",
                             bias, a, b, c)
            margins["layer2"] = max(margins["layer2"], float(mg.max()))

            # fc, from the device's act2
            bias = per_env(v["b3"])
            got = act3[rows]
            pre, absdot = cr.fc_reference(cur["act2"][rows],
                                          cur["w3_fp8"][a:b], v["b3"][a:b])
            ok, mg = _layer(got, pre, absdot, cr.K_FC, "bf16", bias)
            if not bool(ok.all()):
                _raise_layer("fc", got, pre, absdot, cr.K_FC, "bf16", bias,
                             a, b, c)
            margins["fc"] = max(margins["fc"], float(mg.max()))
    rep["margins"] = margins

    # -- head ----------------------------------------------------------------
    rep.update(check_head(prev["state"], prev["racc"], cur["state"],
                          cur["racc"], hd, env_A, env_B, t))

    # -- fitness -------------------------------------------------------------
    fit = cur["fitness"].double().reshape(-1)
    d = (fit - cur["racc"].double().mean(dim=1)).abs()
    if not bool((d <= FIT_TOL).all()):
        m = int(torch.argmax(torch.nan_to_num(d, nan=np.inf)))
        raise StageError("fitness", (
            "member %d: rollout returned %.9g, the mean of its racc row is "
            "%.9g") % (m, fit[m], cur["racc"].double().mean(dim=1)[m]))
    rep["fitness_err_over_tol"] = float(d.max()) / FIT_TOL

    # -- wpert ---------------------------------------------------------------
    if perturb_members is not None:
        rep["wpert_margin"], rep["neighbour_miss"] = check_perturbation(
            cur, const["theta"].cpu(), const["sigma"], seed, it,
            const["rank"], const["pop_per_gpu"], perturb_members,
            pairs_total=const["pop_per_gpu"] * const.get("world", 1) // 2)
    return rep


def chunk_corner_members(pop, chunks):
    """First and last member of the first and of the last chunk."""
    per = pop // chunks
    return sorted({0, per - 1, pop - per, pop - 1})


def format_report(name, h, rep):
    m = rep["margins"]
    return ("%s step %d: margins l1 %.4f l2 %.4f fc %.4f; decided %d "
            "undecided %d actions %s min gap/bound %.1f; state %.4f racc "
            "%.4f fitness %.4f of tol; wpert %s; ambiguous obs pixels %d, "
            "envs closer to the fma / the two-rounding evaluation %d / %d" % (
                name, h, m["layer1"], m["layer2"], m["fc"], rep["decided"],
                rep["undecided"], rep["actions"], rep["min_gap_over_bound"],
                rep["state_err_over_tol"], rep["racc_err_over_tol"],
                rep["fitness_err_over_tol"],
                "%.4f (neighbour misses %.4f)" % (
                    rep["wpert_margin"], rep["neighbour_miss"])
                if "wpert_margin" in rep else "n/a",
                rep["ambiguous_pixels"], rep["fused_envs"],
                rep["unfused_envs"]))


# ---------------------------------------------------------------------------
# fp32 emulation of ConvESEngine (CPU tests and the seed search only)
# ---------------------------------------------------------------------------

MUTATIONS = (
    "chunk1_reads_chunk0_znoise", "chunk1_uses_chunk0_znoise",
    "noise_t_plus_1", "noise_at_capture_iteration",
    "member_offset_drops_m0", "member_offset_drops_rank",
    "racc_sliced_at_m0_times_E", "racc_assigned", "racc_not_reset",
    "state_reinitialised_each_step", "state_not_written_back",
    "antithetic_signs_swapped",
)


@functools.lru_cache(maxsize=40)
def _pair_noise32(seed, iteration, pair):
    return philox_ref.noise_for_pair(seed, iteration, pair, cr.NP_CONV)


def emu_head(act3, wpert, state, racc, env_A, env_B, last_max=False):
    """conv_head_env in fp32 for members wpert[M]: returns (state, racc)."""
    import test_conv_reference as tcr

    m = wpert.shape[0]
    w4 = wpert[:, cr.OFF_W4:cr.OFF_B4].float().reshape(m, 6, 256)
    b4 = wpert[:, cr.OFF_B4:cr.NP_CONV].float()
    h = act3.float().reshape(m, E, 256)
    logits = (torch.einsum("mek,mak->mea", h, w4) + b4[:, None, :]).reshape(
        m * E, 6).numpy()
    if last_max:
        action = 5 - logits[:, ::-1].argmax(axis=1)
    else:
        action = logits.argmax(axis=1)  # first maximum
    force = (torch.from_numpy(action.copy()).float() - 2.5) * 0.4
    s = state.float()
    drive = tcr.fast_tanh32(s @ env_A.float().T)
    snew = 0.97 * s + 0.08 * drive + 0.05 * env_B.float() * force[:, None]
    return snew, racc.reshape(-1) + (1.0 - 0.1 * (snew * snew).sum(dim=1))


class EmuEngine:
    """ConvESEngine's buffers and ``_rollout_body`` in fp32 torch / numpy,
    chunks run one after the other as eager launches on one stream would.
    Unwritten memory holds 7."""

    def __init__(self, case, horizon, mutation=None, fused=False):
        from fiber_amd.es import conv_policy
        from fiber_amd.es.engine import make_env_params

        self.case, self.h, self.mut = case, horizon, mutation
        self.fused = fused
        cpu = torch.device("cpu")
        seed, pop = case["seed"], case["pop"]
        self.theta = conv_policy.init_conv_theta(seed, cpu)
        self.env_A, self.env_B = make_env_params(seed, cpu)
        self.gtab_bf = conv_policy.make_gtab(seed, cpu).to(torch.bfloat16)
        self.wpert = torch.full((pop, cr.NP_CONV_PAD), 7.0).to(torch.bfloat16)
        self.w1_fp8 = torch.zeros(pop, 4096, dtype=torch.uint8)
        self.w3_fp8 = torch.zeros(pop, 256 * cr.K_FC, dtype=torch.uint8)
        self.act1 = torch.zeros(pop * E, 6400, dtype=torch.bfloat16)
        self.act2 = torch.zeros(pop * E, cr.K_FC, dtype=torch.uint8)
        self.act3 = torch.zeros(pop * E, 256, dtype=torch.bfloat16)
        self.state = torch.full((pop * E, 4), 7.0)
        # room for the rows a mis-sliced racc pointer would reach
        self.racc_buf = torch.full((pop * E + pop, E), 7.0)
        self.znoise = torch.full((case["chunks"], NOISE_BYTES), 0x7F,
                                 dtype=torch.uint8)
        self.captured = None

    def const(self, t):
        c = self.case
        return dict(seed=c["seed"], iteration=c["iteration"], t=t,
                    chunks=c["chunks"], gtab_bf=self.gtab_bf,
                    env_A=self.env_A, env_B=self.env_B, theta=self.theta,
                    sigma=SIGMA, rank=c["rank"], world=c["world"],
                    pop_per_gpu=c["pop"], capture=c["capture"])

    def _perturb(self, it, member_offset, m0, n):
        th = self.theta.numpy()
        for k in range(n // 2):
            pair = (member_offset + 2 * k) >> 1
            sz = np.float32(SIGMA) * _pair_noise32(self.case["seed"], it, pair)
            vp, vm = th + sz, th - sz
            if self.mut == "antithetic_signs_swapped":
                vp, vm = vm, vp
            for m, val in ((m0 + 2 * k, vp), (m0 + 2 * k + 1, vm)):
                val = torch.from_numpy(val)
                self.wpert[m, :cr.NP_CONV] = val.to(torch.bfloat16)
                self.w1_fp8[m] = cr.e4m3_bytes(val[:cr.OFF_B1])
                self.w3_fp8[m] = cr.e4m3_bytes(val[cr.OFF_W3:cr.OFF_B3])

    def _chunk(self, half, it):
        import test_conv_reference as tcr

        c, mut = self.case, self.mut
        seed = c["seed"]
        n = c["pop"] // c["chunks"]
        m0 = half * n
        rows = slice(m0 * E, (m0 + n) * E)
        off = c["rank"] * c["pop"] + m0
        if mut == "member_offset_drops_m0":
            off = c["rank"] * c["pop"]
        elif mut == "member_offset_drops_rank":
            off = m0
        r0 = m0 * E if mut == "racc_sliced_at_m0_times_E" else m0
        racc = self.racc_buf[r0:r0 + n]
        self._perturb(it, off, m0, n)
        init = torch.from_numpy(philox_ref.env_init_state(seed, it, E)).repeat(
            n, 1)
        self.state[rows] = init
        if mut != "racc_not_reset":
            racc[:] = 0.0
        it_noise = it
        if mut == "noise_at_capture_iteration":
            it_noise = self.captured
        zw = 0 if mut == "chunk1_uses_chunk0_znoise" else half
        zr = 0 if mut in ("chunk1_uses_chunk0_znoise",
                          "chunk1_reads_chunk0_znoise") else half
        wp = self.wpert[m0:m0 + n]
        for t in range(self.h):
            tn = t + 1 if mut == "noise_t_plus_1" else t
            self.znoise[zw] = noise_mirror(seed, it_noise, tn).reshape(-1)
            st = init if mut == "state_reinitialised_each_step" \
                else self.state[rows].clone()
            obs = cr.obs_reference(self.znoise[zr], st, self.gtab_bf,
                                   fused=self.fused)
            w1 = cr.e4m3_val(self.w1_fp8[m0:m0 + n]).reshape(n, 16, 8, 8, 4)
            a1 = tcr.emulate(obs, w1, wp[:, cr.OFF_B1:cr.OFF_W2], 4, "bf16")
            a2 = tcr.emulate(
                a1.float().reshape(n * E, 20, 20, 16),
                wp[:, cr.OFF_W2:cr.OFF_B2].float().reshape(n, 32, 4, 4, 16),
                wp[:, cr.OFF_B2:cr.OFF_W3], 2, "e4m3")
            a3 = tcr.emulate(
                cr.e4m3_val(a2).reshape(n * E, 9, 9, 32),
                cr.e4m3_val(self.w3_fp8[m0:m0 + n]).reshape(n, 256, 9, 9, 32),
                wp[:, cr.OFF_B3:cr.OFF_W4], 1, "bf16")
            self.act1[rows] = a1.reshape(n * E, -1)
            self.act2[rows] = a2.reshape(n * E, -1)
            self.act3[rows] = a3.reshape(n * E, -1)
            snew, rnew = emu_head(a3, wp, st, racc, self.env_A, self.env_B)
            if mut != "state_not_written_back":
                self.state[rows] = snew
            if mut == "racc_assigned":
                rnew = rnew - racc.reshape(-1)
            racc[:] = rnew.reshape(n, E)

    def rollout(self, it):
        if self.captured is None:
            self.captured = it
        for half in range(self.case["chunks"]):
            self._chunk(half, it)
        return self.buffers()

    def run(self):
        """The case's call sequence: the capturing call, then the checked
        iteration."""
        if self.case["capture"] is not None:
            self.rollout(self.case["capture"])
        return self.rollout(self.case["iteration"])

    def buffers(self):
        racc = self.racc_buf[:self.case["pop"]].clone()
        return dict(wpert=self.wpert.clone(), w1_fp8=self.w1_fp8.clone(),
                    w3_fp8=self.w3_fp8.clone(), znoise=self.znoise.clone(),
                    act1=self.act1.clone(), act2=self.act2.clone(),
                    act3=self.act3.clone(), state=self.state.clone(),
                    racc=racc, fitness=racc.mean(dim=1))


def emulate_case(case, mutation=None, horizons=None, fused=False):
    """{h: buffers} for h = 0 .. max horizon of the case."""
    hs = horizons or range(0, max(case["horizons"]) + 1)
    return {h: EmuEngine(case, h, mutation, fused).run() for h in hs}


def search_seed(name, first=1, last=200):
    """First seed at which, under the fp32 emulation, every env of every
    checked step of the case has gap > 4x its largest bound and the
    actions of the case take >= 4 distinct values.  Prints every seed
    tried."""
    for seed in range(first, last + 1):
        case = dict(CASES[name], seed=seed)
        ratio, actions = np.inf, set()
        for h in case["horizons"]:
            cur = EmuEngine(case, h).run()
            v = cr.policy_views(cur)
            hd = head_decisions(cur["act3"], v["w4"], v["b4"])
            ratio = min(ratio, float(hd["gap_over_bound"].min()))
            actions |= set(hd["action"].tolist())
        ok = ratio > 4 and len(actions) >= 4
        print("%s seed %d: min gap/bound %.2f, actions %s -> %s"
              % (name, seed, ratio, sorted(actions),
                 "ok" if ok else "rejected"), flush=True)
        if ok:
            return seed, ratio
    raise RuntimeError("no seed found")


if __name__ == "__main__":
    import sys

    for case_name in sys.argv[1:] or list(CASES):
        search_seed(case_name)
