"""The low-rank perturbation kernels (fiber_amd/csrc/ops/lowrank_kernels.hip)
and LMMAESEngine (fiber_amd/es/lmmaes.py) on the device.

  parameters   es_perturb_lowrank against lmmaes_oracle.lowrank_params,
               element by element within the bound that function derives
  rollout      J = 0: the bits of es_rollout_mlp.  J > 0: the bits of
               es_rollout_mlp_pairs at sigma = 0 on the perturbed rows
               (documented as bit-identical to the rollout), obs_stat[:8]
               within 9 U sum|partials| of their float64 sum (the depth of
               obs_stat_reduce's tree for up to 256 members: one add in the
               thread, 8 levels), the count exact
  engine       three steps against lmmaes_oracle.step_fp64 fed the device's
               fitness, within its bounds; checkpoints bit for bit
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(
    __file__))))
import lmmaes_cases as C  # noqa: E402
import rollout_oracle_cases as RC  # noqa: E402
from fiber_amd.es import lmmaes_oracle as oracle  # noqa: E402
from fiber_amd.es import philox_ref  # noqa: E402
from fiber_amd.es.rollout_oracle import U  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X")]


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to("cuda:0").contiguous()


def _inputs(J):
    """theta, dirs, mix and (mu, nu, A, B), on the device."""
    theta, mu, nu, A, B = (_dev(a) for a in RC.member_args())
    dirs, mix = (_dev(a) for a in C.lowrank_inputs(J))
    return theta, dirs, mix, (mu, nu, A, B)


@pytest.mark.parametrize("pop,offset", C.LAUNCHES)
@pytest.mark.parametrize("J", C.DIRS)
def test_perturbed_parameters_against_the_oracle(J, pop, offset):
    from fiber_amd import ops

    theta, dirs, mix, _ = _inputs(J)
    got = ops.es_perturb_lowrank(theta, C.SIGMA, dirs, mix, C.SCALE, C.SEED,
                                 C.ITER, offset, pop)
    again = ops.es_perturb_lowrank(theta, C.SIGMA, dirs, mix, C.SCALE,
                                   C.SEED, C.ITER, offset, pop)
    assert got.shape == (pop, ops.NPARAMS) and torch.equal(got, again)
    got = got.cpu().double().numpy()
    for i in range(pop):        # both members of every pair
        member = offset + i
        z = philox_ref.noise_for_pair(C.SEED, C.ITER, member // 2,
                                      ops.NPARAMS)
        sgn = np.float32(-C.SIGMA if member % 2 else C.SIGMA)
        want, bound = oracle.lowrank_params(
            theta.cpu().numpy(), sgn, z, dirs.cpu().numpy(),
            mix.cpu().numpy(), C.SCALE)
        err = np.abs(got[i] - want)
        assert np.all(err <= bound), (member, int(np.argmax(err / bound)))
        for j in (4608, 4609):  # the tail block
            assert err[j] <= bound[j], (member, j)
        # the perturbation is there, and far above the bound
        assert np.abs(want - theta.cpu().numpy()).mean() > 1e2 * bound.mean()


@pytest.mark.parametrize("pop,offset", C.LAUNCHES)
def test_no_directions_gives_the_isotropic_kernels_bits(pop, offset):
    from fiber_amd import ops

    theta, dirs, mix, env = _inputs(0)
    fit, stat = ops.es_rollout_mlp_lowrank(
        theta, C.SIGMA, dirs, mix, 1.0, C.SEED, C.ITER, C.HORIZON, offset,
        pop, *env)
    want_fit, want_stat = ops.es_rollout_mlp(
        theta, C.SIGMA, C.SEED, C.ITER, C.HORIZON, offset, pop, *env)
    assert torch.equal(fit, want_fit) and torch.equal(stat, want_stat)


@pytest.mark.parametrize("pop,offset", C.LAUNCHES)
@pytest.mark.parametrize("J", [J for J in C.DIRS if J])
def test_rollout_runs_the_perturbed_parameters(J, pop, offset):
    from fiber_amd import ops

    theta, dirs, mix, env = _inputs(J)
    fit, stat = ops.es_rollout_mlp_lowrank(
        theta, C.SIGMA, dirs, mix, C.SCALE, C.SEED, C.ITER, C.HORIZON,
        offset, pop, *env)
    params = ops.es_perturb_lowrank(theta, C.SIGMA, dirs, mix, C.SCALE,
                                    C.SEED, C.ITER, offset, pop)
    rows = [t.expand(pop, *t.shape).contiguous() for t in env]
    row_fit, row_stat = ops.es_rollout_mlp_pairs(
        params, 0.0, ops.pair_seeds([C.SEED] * pop, theta.device), C.ITER,
        C.HORIZON, 2, *rows)
    assert torch.equal(fit, row_fit[:, 0])
    # sigma = 0 makes both members of a row the same member
    part = row_stat[:, :8].cpu().double().numpy() / 2.0
    err = np.abs(stat[:8].cpu().double().numpy() - part.sum(axis=0))
    assert np.all(err <= 9.0 * U * np.abs(part).sum(axis=0))
    assert float(stat[8]) == pop * 64 * C.HORIZON
    # ... and not the unperturbed or the isotropic one
    iso = ops.es_rollout_mlp(theta, C.SIGMA, C.SEED, C.ITER, C.HORIZON,
                             offset, pop, *env)[0]
    assert not torch.equal(fit, iso)


def _engine(pop=8):
    from fiber_amd.es import ESConfig, LMMAESEngine

    return LMMAESEngine(ESConfig(pop_per_gpu=pop, horizon=C.HORIZON,
                                 seed=C.SEED), device=torch.device("cuda", 0))


def _state(eng):
    return {"theta": eng.theta.cpu().numpy(), "sigma": eng.sigma,
            "p_sigma": eng.p_sigma.cpu().numpy(),
            "dirs": eng.dirs.cpu().numpy(), "t_step": eng.t_step}


def test_engine_steps_against_the_oracle(tmp_path):
    from fiber_amd import ops

    eng, other = _engine(), _engine()
    for want_active in (0, 1, 2):
        before = _state(eng)
        active, scale, mix = eng.sampling()
        fitness, _ = ops.es_rollout_mlp_lowrank(
            eng.theta, eng.sigma, active, mix.float(), scale, C.SEED,
            eng.t_step, C.HORIZON, 0, 8, eng.obs_mu, eng.obs_nu, eng.env_A,
            eng.env_B)
        stats = eng.step()
        assert stats["n_active"] == want_active == active.shape[0]
        assert stats["sigma"] == eng.sigma
        new, tol = oracle.step_fp64(before, fitness.cpu().numpy(), eng.cfg,
                                    eng.lm, before["t_step"])
        got = _state(eng)
        assert got["t_step"] == new["t_step"]
        for key, bound in tol.items():
            err = np.abs(np.asarray(got[key], dtype=np.float64) - new[key])
            assert np.all(err <= bound), key
        assert np.abs(new["theta"] - before["theta"]).max() > 0.0
    assert np.all(np.abs(eng.dirs.cpu().numpy()).max(axis=1) > 0.0)

    # save, load into a fresh engine, step both: every tensor bit for bit
    eng.save(str(tmp_path / "lmmaes.pt"))
    other.load(str(tmp_path / "lmmaes.pt"))
    assert eng.step() == other.step()
    for key, value in eng.state_dict().items():
        if torch.is_tensor(value):
            assert torch.equal(value, other.state_dict()[key]), key
        else:
            assert value == other.state_dict()[key], key
    assert torch.equal(eng.sample(3), other.sample(3))


def test_bad_arguments_raise_before_any_launch():
    from fiber_amd import ops
    from fiber_amd.es import ESConfig, LMMAESEngine

    with pytest.raises(NotImplementedError):
        LMMAESEngine(ESConfig(pop_per_gpu=8), ctx=object())
    theta, dirs, mix, env = _inputs(3)
    tail = (C.SEED, C.ITER, C.HORIZON, 0, 2) + env
    wide = torch.zeros(33, ops.NPARAMS, device="cuda:0")
    for bad_dirs, bad_mix, error in (
            (dirs[:, :-1].contiguous(), mix, ValueError),
            (dirs, mix[:2, :2].contiguous(), ValueError),
            (wide, torch.zeros(33, 33, device="cuda:0"), ValueError),
            (dirs.reshape(-1)[1:1 + 2 * ops.NPARAMS].view(2, -1),
             mix[:2, :2].contiguous(), ValueError),      # misaligned
            (dirs.double(), mix, TypeError),
            (dirs, mix.t(), TypeError),
            (dirs.cpu(), mix, TypeError)):
        with pytest.raises(error):
            ops.es_rollout_mlp_lowrank(theta, C.SIGMA, bad_dirs, bad_mix,
                                       C.SCALE, *tail)
        with pytest.raises(error):
            ops.es_perturb_lowrank(theta, C.SIGMA, bad_dirs, bad_mix,
                                   C.SCALE, C.SEED, C.ITER, 0, 2)
    for offset, pop in ((1, 2), (0, 3)):
        with pytest.raises(ValueError):
            ops.es_rollout_mlp_lowrank(
                theta, C.SIGMA, dirs, mix, C.SCALE, C.SEED, C.ITER,
                C.HORIZON, offset, pop, *env)
    with pytest.raises(ValueError):
        ops.es_perturb_lowrank(theta, C.SIGMA, dirs, mix, float("nan"),
                               C.SEED, C.ITER, 0, 2)
