"""The MLP rollout loop one step at a time at long horizons, and with the
+-5 clamp of the normalised obs active (tests/rollout_step_cases.py;
derivations in profiles/rollout_oracle.md, "One step at a time").

The kernel's own fp32 state at horizon h, ``final_states`` of es_eval_bc /
es_rollout_mlp_bc, starts ONE step of the fp64 oracle, which is compared
with the kernel's state at h + 1.  Nothing accumulates over earlier steps,
so the bound is the one-step state bound, 3e-7 to 9e-7, at h = 8, 49, 50
and 199 alike.  No env is exempt: where the oracle calls the step decided
the kernel must have its outcome, elsewhere one of the two outcomes the
env step has.

  state       |final_{h+1} - states[:, 1]| <= state_err[:, 1], per dim
  reward      |(ep_{h+1} - ep_h) - reward[:, 0]|
              <= return_tol[:, 0] + 7 U (h + 1) (1 + 0.4 s_max^2)
  obs_stat    |(stat_{h+1} - stat_h) - sum final_h| <= U (depth_h abs_h
              + depth_{h+1} abs_{h+1}), abs from the kernel's sumsq slots
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(
    __file__))))
import rollout_oracle_cases as C  # noqa: E402
import rollout_step_cases as S  # noqa: E402
from fiber_amd.es import rollout_oracle as oracle  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

U = oracle.U


def _np(t):
    return t.cpu().numpy().copy()


@pytest.fixture(scope="module")
def eval_runs():
    """{(set, horizon): (scores[K][M], final[K][M][64][4], episodes[K][M]
    [64])} of es_eval_bc, fp32 on the host, for every horizon a case needs:
    twelve launches of four blocks."""
    from fiber_amd import ops

    need = {name: set() for name in S.SETS}
    for name, h in S.STEP_CASES:
        need[name] |= {h, h + 1}
    need["clamp"] |= set(S.CLAMP_HORIZONS)
    got = {}
    for name in S.SETS:
        inp = S.inputs_torch(name, torch.device("cuda", 0))
        for h in sorted(need[name]):
            scores, _bc, final, ep = ops.es_eval_bc(
                *inp, C.SEED, C.ITER, h, return_final_states=True,
                return_episodes=True)
            got[(name, h)] = (_np(scores), _np(final), _np(ep))
    return got


def _cell_s_max(eval_runs, name, k, m):
    """Largest |state| the kernel reported for the cell at any horizon."""
    return max(float(np.abs(v[1][k, m]).max())
               for (n, _h), v in eval_runs.items() if n == name)


@requires_gpu
@pytest.mark.parametrize("name,h", S.STEP_CASES)
def test_eval_one_step_states_and_rewards(eval_runs, name, h):
    """Every env of every cell: the state at h + 1 is the oracle's step
    from the kernel's state at h, and the episode returns of the two
    launches differ by that step's reward."""
    _s, final_h, ep_h = eval_runs[(name, h)]
    _s, final_h1, ep_h1 = eval_runs[(name, h + 1)]
    assert np.isfinite(final_h1).all() and np.isfinite(ep_h1).all()
    bad = []
    for k, m in S.CELLS:
        st = S.one_step(S.cell_args(name, k, m), final_h[k, m])
        share = float(st.decided.mean())
        sm = S.match_states(st, final_h1[k, m])
        err, tol = S.match_reward(st, sm, ep_h[k, m], ep_h1[k, m], h,
                                  _cell_s_max(eval_runs, name, k, m))
        print("%s h=%d cell(%d,%d): decided %.3f, other outcome taken by %d "
              "undecided, state max err/tol %.3f (bound %.2e), reward max "
              "err %.2e err/tol %.3f (tol %.2e)"
              % (name, h, k, m, share, int(sm.took_alt.sum()),
                 sm.ratio.max(), st.main.state_err[:, 1].max(), err.max(),
                 (err / tol).max(), tol.max()))
        assert share >= S.CAP, (name, h, k, m, share)
        if name == "clamp":
            hi, lo, mixed, hi_share, lo_share = S.clamp_condition(st.x_raw)
            print("   x above +5 per dim %s, below -5 %s"
                  % (np.round(hi_share, 3), np.round(lo_share, 3)))
            assert hi and lo and mixed, (k, m)
        for what, ok in (("state", sm.ok), ("reward", err <= tol)):
            if not ok.all():
                bad.append((what, (k, m), np.flatnonzero(~ok).tolist()))
    assert not bad, bad


@requires_gpu
def test_clamp_set_multi_step(eval_runs):
    """The multi-step comparison of test_rollout_oracle_gpu.py (episodes,
    scores) and the final states, on the clamp-active set at h = 1, 2, 3,
    on every episode decided through h: at least 90% of each cell."""
    th, mu, nu, _A, _B = S.inputs_numpy("clamp")
    s0, _e = oracle.init_states(C.SEED, C.ITER)
    for k, m in S.CELLS:
        ro = S.clamp_cell(k, m)
        # the states the kernel normalised: s_0 and its own s_1, s_2
        seen = [s0] + [eval_runs[("clamp", h)][1][k, m]
                       for h in S.CLAMP_HORIZONS[:-1]]
        rstd = 1.0 / np.sqrt(nu[k].astype(np.float64) + oracle.C1EM4)
        x = (np.stack(seen).astype(np.float64)
             - mu[k].astype(np.float64)) * rstd
        hi, lo, mixed, hi_share, lo_share = S.clamp_condition(x)
        assert hi and lo and mixed, (k, m)
        assert hi_share[2:].max() == 0.0 and lo_share[2:].max() == 0.0
        for h in S.CLAMP_HORIZONS:
            scores, final, ep = eval_runs[("clamp", h)]
            dec = ro.decided[:, h - 1]
            assert dec.mean() >= C.CAP_SHORT, (k, m, h)
            e_ep = np.abs(ep[k, m].astype(np.float64) - ro.returns[:, h - 1])
            t_ep = ro.return_tol[:, h - 1]
            e_s = np.abs(final[k, m].astype(np.float64) - ro.states[:, h])
            t_s = ro.state_err[:, h]
            print("clamp h=%d cell(%d,%d): compared %d/64, episodes max "
                  "err/tol %.3f, states max err/tol %.3f; x above +5 %s "
                  "below -5 %s"
                  % (h, k, m, int(dec.sum()), (e_ep[dec] / t_ep[dec]).max(),
                     (e_s[dec] / t_s[dec]).max(), np.round(hi_share, 3),
                     np.round(lo_share, 3)))
            assert (e_ep[dec] <= t_ep[dec]).all(), (
                k, m, h, np.flatnonzero(dec & (e_ep > t_ep)).tolist())
            assert (e_s[dec] <= t_s[dec]).all(), (
                k, m, h, np.flatnonzero(dec & (e_s > t_s).any(-1)).tolist())
            want = np.where(dec, ro.returns[:, h - 1], ep[k, m]).mean()
            tol = (t_ep[dec].sum() / 64.0
                   + 6.0 * U * np.abs(ep[k, m]).mean())
            assert abs(float(scores[k, m]) - want) <= tol, (k, m, h)


# ---- perturbed members ------------------------------------------------------

def _device_member_args():
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(a).to(dev).contiguous()
            for a in C.member_args()]


@pytest.fixture(scope="module")
def member_runs():
    """{(sigma, horizon): (fitness[POP], obs_stat[9], final[POP][64][4])}
    of es_rollout_mlp_bc, one launch of POP members at MEMBER_OFFSET."""
    from fiber_amd import ops

    theta, mu, nu, A, B = _device_member_args()
    got = {}
    for sigma in C.SIGMAS:
        seed = S.MEMBER_SEEDS[sigma]
        for h in sorted({x for h in S.MEMBER_H for x in (h, h + 1)}):
            fit, stat, _bc, final = ops.es_rollout_mlp_bc(
                theta, sigma, seed, C.ITER, h, S.MEMBER_OFFSET, C.POP, mu,
                nu, A, B, return_final_states=True)
            got[(sigma, h)] = (_np(fit), _np(stat), _np(final))
    return got


@requires_gpu
@pytest.mark.parametrize("sigma", C.SIGMAS)
@pytest.mark.parametrize("h", S.MEMBER_H)
def test_members_one_step(member_runs, h, sigma):
    """Members 3..6 of one launch (an antithetic pair split at each end):
    every env's state at h + 1 against one oracle step of the member's
    perturbed policy from the kernel's state at h.  es_rollout_mlp_bc
    returns no episodes; the fitness, their mean, moves by the mean
    reward: the per-env bound averaged, plus 6 U mean|episode| for the
    shuffle tree of each launch."""
    seed = S.MEMBER_SEEDS[sigma]
    fit_h, _st, final_h = member_runs[(sigma, h)]
    fit_h1, _st, final_h1 = member_runs[(sigma, h + 1)]
    assert np.isfinite(final_h1).all() and np.isfinite(fit_h1).all()
    bad = []
    for i in range(C.POP):
        member = S.MEMBER_OFFSET + i
        st = S.one_step(S.member_step_args(sigma, seed, member), final_h[i])
        share = float(st.decided.mean())
        sm = S.match_states(st, final_h1[i])
        s_max = max(float(np.abs(v[2][i]).max())
                    for (sg, _h), v in member_runs.items() if sg == sigma)
        want = np.where(sm.took_alt, st.alt.reward[:, 0],
                        st.main.reward[:, 0]).mean()
        p1 = S.partial_bound(h + 1, s_max)
        tol = (S.reward_tol(st, sm.took_alt, h, s_max).mean()
               + 12.0 * U * p1)
        err = abs((float(fit_h1[i]) - float(fit_h[i])) - want)
        print("sigma=%g h=%d member %d: decided %.3f, other outcome taken "
              "by %d undecided, state max err/tol %.3f (bound %.2e), "
              "fitness step err %.2e err/tol %.3f"
              % (sigma, h, member, share, int(sm.took_alt.sum()),
                 sm.ratio.max(), st.main.state_err[:, 1].max(), err,
                 err / tol))
        assert share >= S.CAP, (sigma, h, member, share)
        if not sm.ok.all():
            bad.append(("state", member, np.flatnonzero(~sm.ok).tolist()))
        if not err <= tol:
            bad.append(("fitness", member, err, tol))
    assert not bad, bad


@requires_gpu
@pytest.mark.parametrize("sigma", C.SIGMAS)
def test_obs_stat_step_at_the_production_horizon(member_runs, sigma):
    """obs_stat[:8] of es_rollout_mlp at h + 1 and at h differ by the states
    s_h of every member and env, the _bc sibling's final_h, for h = 199 and
    200; obs_stat[8] is 64 * POP * horizon exactly."""
    from fiber_amd import ops

    theta, mu, nu, A, B = _device_member_args()
    seed = S.MEMBER_SEEDS[sigma]
    stat = {}
    for hor in sorted({x for h in S.STAT_H for x in (h, h + 1)}):
        _fit, st = ops.es_rollout_mlp(theta, sigma, seed, C.ITER, hor,
                                      S.MEMBER_OFFSET, C.POP, mu, nu, A, B)
        stat[hor] = _np(st).astype(np.float64)
        assert stat[hor][8] == 64 * C.POP * hor, (hor, stat[hor][8])
    finals = {h: member_runs[(sigma, h)][2] for h in (199, 200)}
    assert set(S.STAT_H) == set(finals)
    for h in S.STAT_H:
        # the sibling's statistics are the same bits
        if (sigma, h) in member_runs:
            assert np.array_equal(member_runs[(sigma, h)][1].astype(
                np.float64), stat[h])
        want, absw = S.stat_step_want(finals[h])
        tol = S.stat_step_tol(stat[h], stat[h + 1], absw, h,
                              C.POP * oracle.ENVS)
        err = np.abs((stat[h + 1][:8] - stat[h][:8]) - want)
        print("sigma=%g h=%d: obs_stat step max err/tol %.3f; err %s tol %s "
              "want %s" % (sigma, h, (err / tol).max(), np.round(err, 4),
                           np.round(tol, 3), np.round(want, 2)))
        assert (err <= tol).all(), (h, err, tol)
