"""The MLP rollout kernels against the per-episode fp64 oracle
(fiber_amd/es/rollout_oracle.py; derivations in profiles/rollout_oracle.md).

The goldens of test_rollout_bits.py were recorded from the kernel itself,
and the fp32 mirrors are compared at 5e-2 on a mean over 64 episodes.
Here every episode that the oracle calls decided (no fp32 rounding in the
kernel can turn one of its actions) is compared on its own.

Tolerance of an episode return at horizon h, ``return_tol[e][h-1]``: with
U = 2^-24 and err_t[d] the bound on the state,

  err_0[d]   = |s_0[d]| * Z_REL                  (libm of the two sides)
  err_t+1[d] = 0.97 err_t[d]
               + 0.08 (EPS_TANH + 4 U sum_e |A[d][e] s[e]|
                       + sum_e |A[d][e]| err_t[e])     (the drive's tanh)
               + U (|0.97 s| + |fma| + |0.05 B| + |s_t+1|)   (4 roundings)
  tol(h) = sum_{t<h, d} [ 0.2 |s_t+1| err_t+1 + 0.1 err_t+1^2
                          + 3 U 0.1 s_t+1^2 + U |r_t[d]|    (reward term)
                          + U |partial sum after step t| ]  (h fp32 adds)
           + 3 U sum_d |partial[d]|              (4 partials -> episode)

It is computed from the oracle's own magnitudes, about 2e-6 per step: 1e-5
at h = 8.  A member's fitness adds 6 U mean|episode| for the 6-level tree
over the 64 returns (the division by 64 is exact).
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(
    __file__))))
import rollout_oracle_cases as C  # noqa: E402
from fiber_amd.es import rollout_oracle as oracle  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

CELLS = [(k, m) for k in range(C.K) for m in range(C.M)]


def _assert_coverage():
    """The coverage conditions, from the oracle alone."""
    seen = {h: np.zeros(64, bool) for h in C.HORIZONS}
    for k, m in CELLS:
        dec = C.cell(k, m).decided
        for h in C.HORIZONS:
            share = dec[:, h - 1].mean()
            if h <= C.CAP_SHORT_H:
                assert share >= C.CAP_SHORT, (k, m, h, share)
            if h <= C.CAP_LONG_H:
                assert share >= C.CAP_LONG, (k, m, h, share)
            seen[h] |= dec[:, h - 1]
    for h in C.HORIZONS:
        # all four column tiles, all 16 lanes of each
        assert seen[h].all(), (h, np.flatnonzero(~seen[h]))


@pytest.fixture(scope="module")
def eval_episodes():
    """es_eval_matrix episodes [K][M][64] per horizon, float64 on the
    host; the coverage conditions are asserted before the first launch."""
    from fiber_amd import ops

    _assert_coverage()
    inp = C.inputs_torch(torch.device("cuda", 0))
    got = {}
    for h in C.HORIZONS:
        scores, ep = ops.es_eval_matrix(*inp, C.SEED, C.ITER, h,
                                        return_episodes=True)
        got[h] = (scores.cpu().double().numpy(), ep.cpu().double().numpy())
    return got


@requires_gpu
def test_eval_matrix_episodes_per_horizon(eval_episodes):
    """Every episode decided through h is within return_tol of the oracle,
    for h = 1, 2, 3, 4, 8 in all K x M cells.  The first departure is
    named by step and env: successive horizons give the per-step reward
    ep_h - ep_(h-1), so the earliest failing horizon brackets the step."""
    first_bad = None
    worst = {}
    for h in C.HORIZONS:
        _scores, ep = eval_episodes[h]
        assert np.isfinite(ep).all()  # the undecided ones included
        for k, m in CELLS:
            ro = C.cell(k, m)
            dec = ro.decided[:, h - 1]
            err = np.abs(ep[k, m] - ro.returns[:, h - 1])
            tol = ro.return_tol[:, h - 1]
            worst[(h, k, m)] = (int(dec.sum()), err[dec].max(),
                                (err[dec] / tol[dec]).max())
            print("h=%d cell(%d,%d): compared %d/64, max |kernel-oracle| "
                  "%.3e, max err/tol %.3f, tol max %.3e"
                  % ((h, k, m) + worst[(h, k, m)] + (tol[dec].max(),)))
            bad = np.flatnonzero(dec & (err > tol))
            if bad.size and first_bad is None:
                prev = [p for p in C.HORIZONS if p < h]
                first_bad = dict(
                    horizon=h, steps="%d..%d" % (prev[-1] if prev else 0,
                                                 h - 1),
                    cell=(k, m), envs=bad.tolist(),
                    kernel=ep[k, m][bad].tolist(),
                    oracle=ro.returns[bad, h - 1].tolist(),
                    tol=tol[bad].tolist())
    assert first_bad is None, first_bad


@requires_gpu
def test_eval_matrix_step_rewards(eval_episodes):
    """The reward of the single steps 1, 2 and 3, as ep_h - ep_(h-1) of
    successive launches, against the oracle's reward term, on episodes
    decided through h.  Each of the two returns is within its own bound."""
    for h in (2, 3, 4):
        ep, prev = eval_episodes[h][1], eval_episodes[h - 1][1]
        for k, m in CELLS:
            ro = C.cell(k, m)
            dec = ro.decided[:, h - 1]
            err = np.abs((ep[k, m] - prev[k, m]) - ro.reward[:, h - 1])
            tol = ro.return_tol[:, h - 1] + ro.return_tol[:, h - 2]
            bad = np.flatnonzero(dec & (err > tol))
            assert bad.size == 0, (
                "step %d, cell %s, envs %s" % (h - 1, (k, m), bad.tolist()),
                err[bad], tol[bad])


@requires_gpu
def test_eval_matrix_scores(eval_episodes):
    """scores[k][m] is the fp32 tree sum of the cell's 64 episodes over 64.
    With the oracle's return on the decided episodes and the kernel's own
    on the others, it is compared as a member's fitness is."""
    for h in C.HORIZONS:
        scores, ep = eval_episodes[h]
        for k, m in CELLS:
            ro = C.cell(k, m)
            dec = ro.decided[:, h - 1]
            want = np.where(dec, ro.returns[:, h - 1], ep[k, m]).mean()
            tol = (ro.return_tol[dec, h - 1].sum() / 64.0
                   + 6.0 * oracle.U * np.abs(ep[k, m]).mean())
            assert abs(scores[k, m] - want) <= tol, (h, k, m)


def _device_member_args():
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(a).to(dev).contiguous()
            for a in C.member_args()]


@requires_gpu
def test_obs_stats_horizon_1_is_the_env_init_draw():
    """At horizon 1 the statistics hold s_0 = 0.3 z only (the prologue
    "phase A"; the t < horizon-1 branch never runs): pop 2."""
    from fiber_amd import ops

    theta, mu, nu, A, B = _device_member_args()
    for sigma, (seed, off, _h) in ((s, C.LAUNCHES[s][0]) for s in C.SIGMAS):
        _fit, stat = ops.es_rollout_mlp(theta, sigma, seed, C.ITER, 1, off,
                                        2, mu, nu, A, B)
        stat = stat.cpu().double().numpy()
        st = oracle.obs_stats(C.launch(sigma, seed, off)[:2], 1)
        want = np.concatenate([st.sum, st.sumsq])
        tol = oracle.obs_stats_tol(st)
        print("h=1 sigma", sigma, "seed", seed, "max |err| / tol",
              (np.abs(stat[:8] - want) / tol).max(), "tol", tol)
        assert (np.abs(stat[:8] - want) <= tol).all(), (stat, want, tol)
        assert stat[8] == 2 * 64


@requires_gpu
@pytest.mark.parametrize("sigma", C.SIGMAS)
@pytest.mark.parametrize("horizon", (2, 3))
def test_members_fitness_and_obs_stats(horizon, sigma):
    """Launches of 4 members (both parities, member_offset 0 and not, one
    that splits an antithetic pair) whose 64 envs the oracle calls decided:
    through horizon-1 steps for the statistics, which hold s_0 ..
    s_(horizon-1), and through horizon steps for the fitness.  sum lands
    in slot [d], sumsq in [4+d]: the four dims differ in mu, nu, env_A and
    env_B, and any two slots differ by over 100 tolerances
    (tests/test_rollout_oracle.py).  sigma = 4.0 is the saturating path."""
    from fiber_amd import ops

    theta, mu, nu, A, B = _device_member_args()
    launches = C.launches_decided_through(sigma, horizon - 1)
    assert len(launches) >= 2
    n_fit = 0
    for seed, off in launches:
        ros = C.launch(sigma, seed, off)
        assert len(ros) == C.POP >= 4
        assert all(ro.decided[:, horizon - 2].all() for ro in ros)
        fit, stat = ops.es_rollout_mlp(theta, sigma, seed, C.ITER, horizon,
                                       off, C.POP, mu, nu, A, B)
        fit = fit.cpu().double().numpy()
        stat = stat.cpu().double().numpy()
        st = oracle.obs_stats(ros, horizon)
        want = np.concatenate([st.sum, st.sumsq])
        tol = oracle.obs_stats_tol(st)
        print("h=%d sigma=%g seed=%d off=%d: stats max err/tol %.3f"
              % (horizon, sigma, seed, off,
                 (np.abs(stat[:8] - want) / tol).max()))
        assert (np.abs(stat[:8] - want) <= tol).all(), (
            seed, off, stat, want, tol)
        assert stat[8] == C.POP * 64 * horizon
        if all(ro.decided[:, horizon - 1].all() for ro in ros):
            for i, ro in enumerate(ros):
                w, t = oracle.fitness_of(ro, horizon)
                print("   member %d fitness err %.3e tol %.3e"
                      % (off + i, abs(fit[i] - w), t))
                assert abs(fit[i] - w) <= t, (seed, off, i, fit[i], w, t)
                n_fit += 1
    assert n_fit >= 2 * C.POP


@requires_gpu
def test_pairs_kernel_fitness_and_obs_stats():
    """es_rollout_mlp_pairs, P = 2, on two fully decided offset-0 launches
    (its own seeds per pair), held to the oracle directly and not only
    through its bit-equality with es_rollout_mlp."""
    from fiber_amd import ops

    theta, mu, nu, A, B = _device_member_args()
    sigma, h, seeds = C.PAIRS_SIGMA, C.PAIRS_H, C.PAIRS_SEEDS
    rep = lambda t: t.unsqueeze(0).repeat(  # noqa: E731
        2, *([1] * t.dim())).contiguous()
    fit, stat = ops.es_rollout_mlp_pairs(
        rep(theta), sigma, ops.pair_seeds(seeds, theta.device), C.ITER, h,
        C.POP, rep(mu), rep(nu), rep(A), rep(B))
    fit = fit.cpu().double().numpy()
    stat = stat.cpu().double().numpy()
    for p, seed in enumerate(seeds):
        ros = C.launch(sigma, seed, 0)
        assert all(ro.decided[:, h - 1].all() for ro in ros)
        for i, ro in enumerate(ros):
            w, t = oracle.fitness_of(ro, h)
            assert abs(fit[p, i] - w) <= t, (p, i, fit[p, i], w, t)
        st = oracle.obs_stats(ros, h)
        want = np.concatenate([st.sum, st.sumsq])
        tol = oracle.obs_stats_tol(st)
        assert (np.abs(stat[p, :8] - want) <= tol).all(), (p, stat[p], want)
        assert stat[p, 8] == C.POP * 64 * h
    assert not np.array_equal(fit[0], fit[1])
