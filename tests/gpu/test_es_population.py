"""GPU tests for the per-pair batched ES ops (es_rollout_mlp_pairs,
centered_rank_pairs, es_grad_pairs) and ESPopulation.

Every pair must get, bit for bit, what the single-pair ops and its own
ESEngine compute, so the oracle chain of those (rollout_reference, the
goldens under tests/golden/) covers the batched path by transitivity.
Thetas, normalisers, environments and seeds differ per pair, so a p-index
mix-up shows; every test also asserts that the pairs' outputs differ.
"""

import dataclasses
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

if torch.cuda.is_available():
    from fiber_amd import ops
    from fiber_amd.es import (ESConfig, ESEngine, ESPopulation,
                              apply_transfers, transfer_matrix)
    from fiber_amd.es import engine as es_engine

REPO = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
SIGMA, ITER = 0.05, 5
# 32-bit patterns with and without the top bit, and one that needs the mask
SEEDS = [1234, 0x9E3779B9, (1 << 32) + 77, 4321, 99, 7, 0xFFFFFFFF, 31337]


def _dev():
    return torch.device("cuda", 0)


def _population(P, device):
    """Distinct thetas, normalisers and envs per pair (the style of
    _population in test_eval_matrix.py)."""
    thetas = torch.stack([es_engine.init_theta(11 + p, "cpu")
                          for p in range(P)])
    nu_vals = [0.5, 1.0, 2.0]
    obs_nu = torch.tensor([[nu_vals[p % 3]] * 4 for p in range(P)])
    obs_mu = torch.tensor([[0.05 * (p + 1), -0.03 * p, 0.02 * p, -0.1]
                           for p in range(P)])
    envs = [es_engine.make_env_params(100 + p, "cpu") for p in range(P)]
    env_A = torch.stack([e[0] for e in envs])
    env_B = torch.stack([e[1] for e in envs])
    return [t.to(device).contiguous()
            for t in (thetas, obs_mu, obs_nu, env_A, env_B)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _run_pairs(pop_in, seeds, horizon, pop):
    thetas, obs_mu, obs_nu, env_A, env_B = pop_in
    return ops.es_rollout_mlp_pairs(
        thetas, SIGMA, ops.pair_seeds(seeds, thetas.device), ITER, horizon,
        pop, obs_mu, obs_nu, env_A, env_B)


def _run_single(pop_in, seeds, p, horizon, pop):
    thetas, obs_mu, obs_nu, env_A, env_B = pop_in
    return ops.es_rollout_mlp(thetas[p], SIGMA, seeds[p], ITER, horizon, 0,
                              pop, obs_mu[p], obs_nu[p], env_A[p], env_B[p])


def _assert_rollout_rows(pop_in, seeds, horizon, pop, fitness, obs_stat):
    P = pop_in[0].shape[0]
    assert fitness.shape == (P, pop) and obs_stat.shape == (P, 9)
    for p in range(P):
        fit, stat = _run_single(pop_in, seeds, p, horizon, pop)
        assert _same_bits(fitness[p], fit), (p, fitness[p], fit)
        assert _same_bits(obs_stat[p], stat), (p, obs_stat[p], stat)
    assert torch.isfinite(fitness).all()
    # pairs and members really differ (else the identity shows nothing)
    assert fitness.flatten().unique().numel() > P * pop // 2
    if P > 1:
        assert obs_stat[:, :8].unique(dim=0).shape[0] == P


@requires_gpu
class TestPairsKernels:
    # 1. rollout, bit
    @pytest.mark.parametrize("P,horizon", [(3, 8), (3, 1), (1, 8)])
    def test_rollout_bit_identical_to_single_pair_kernel(self, P, horizon):
        pop_in = _population(P, _dev())
        seeds = SEEDS[:P]
        fitness, obs_stat = _run_pairs(pop_in, seeds, horizon, 8)
        _assert_rollout_rows(pop_in, seeds, horizon, 8, fitness, obs_stat)
        assert float(obs_stat[0, 8]) == 8 * 64 * horizon

    # 2. stat-reduce stride and ragged grad chunks, bit
    def test_stat_stride_rank_and_ragged_grad_chunks(self):
        P, pop, horizon = 2, 520, 2
        dev = _dev()
        pop_in = _population(P, dev)
        seeds = SEEDS[1:1 + P]
        fitness, obs_stat = _run_pairs(pop_in, seeds, horizon, pop)
        _assert_rollout_rows(pop_in, seeds, horizon, pop, fitness, obs_stat)

        # ranks, plus a row with ties (index-order tie-break): values
        # repeated in blocks, and +-0.0, which compare equal
        tied = (torch.arange(pop, device=dev) % 7).float() - 3.0
        tied[5], tied[200] = 0.0, -0.0
        fit3 = torch.cat([fitness, tied[None]]).contiguous()
        ranks = ops.centered_rank_pairs(fit3)
        assert ranks.shape == (3, pop)
        for p in range(3):
            assert _same_bits(ranks[p], ops.centered_rank(fit3[p])), p
            # the torch reference divides on the CPU: values in [-0.5, 0.5]
            # one fp32 ulp (6e-8) apart at most, ranks are 1/519 apart
            assert torch.allclose(ranks[p].cpu(),
                                  ops.centered_rank_ref(fit3[p].cpu()),
                                  rtol=0, atol=1e-6), p
            # a permutation of the n rank values: no two indices tie
            assert ranks[p].unique().numel() == pop
        assert not torch.equal(ranks[0], ranks[1])

        # 260 Philox pairs: 32 chunks of 9, the last three of them empty
        assert ops._OPS.es_grad_chunks(pop // 2, ops.NPARAMS) == 32
        wpair = (ranks[:P, 0::2] - ranks[:P, 1::2]).contiguous()
        wpair[1, 3] = 0.0  # the w == 0 skip
        sd = ops.pair_seeds(seeds, dev)
        grad = ops.es_grad_pairs(wpair, sd, ITER)
        assert grad.shape == (P, ops.NPARAMS)
        for p in range(P):
            want = ops.es_grad(wpair[p], 0, pop // 2, seeds[p], ITER, dev)
            assert _same_bits(grad[p], want), p
        assert torch.isfinite(grad).all() and grad.norm(dim=1).min() > 0
        assert not torch.equal(grad[0], grad[1])

    # 3. small-population grad (single-chunk branch), bit
    def test_small_population_grad_single_chunk(self):
        P, npairs = 3, 4
        dev = _dev()
        assert ops._OPS.es_grad_chunks(npairs, ops.NPARAMS) == 1
        gen = torch.Generator().manual_seed(5)
        wpair = torch.randn(P, npairs, generator=gen).to(dev)
        seeds = SEEDS[:P]
        grad = ops.es_grad_pairs(wpair, ops.pair_seeds(seeds, dev), ITER)
        for p in range(P):
            want = ops.es_grad(wpair[p], 0, npairs, seeds[p], ITER, dev)
            assert _same_bits(grad[p], want), p
        assert grad.norm(dim=1).min() > 0
        assert grad.unique(dim=0).shape[0] == P

    # 4. full residency, bit
    def test_full_residency_matches_per_pair_launches(self):
        P, pop, horizon = 8, 512, 3
        pop_in = _population(P, _dev())
        fitness, obs_stat = _run_pairs(pop_in, SEEDS, horizon, pop)
        _assert_rollout_rows(pop_in, SEEDS, horizon, pop, fitness, obs_stat)
        assert (obs_stat[:, 8] == float(pop * 64 * horizon)).all()

    # 5. independent oracle
    def test_fitness_vs_fp32_reference(self):
        P, pop, horizon = 2, 4, 8
        pop_in = _population(P, _dev())
        thetas, obs_mu, obs_nu, env_A, env_B = pop_in
        seeds = SEEDS[:P]
        fitness, _stat = _run_pairs(pop_in, seeds, horizon, pop)
        torch.cuda.synchronize()
        refs = []
        for p in range(P):
            ref = es_engine.rollout_reference(
                thetas[p], SIGMA, seeds[p], ITER, horizon, list(range(pop)),
                obs_mu[p], obs_nu[p], env_A[p], env_B[p])
            err = (fitness[p].cpu() - ref).abs().max().item()
            print("pair %d: max |fitness - oracle| = %.3e" % (p, err))
            # the bound of tests/gpu/test_es.py for this shape
            assert err < 5e-2, (p, fitness[p].cpu(), ref)
            refs.append(ref)
        assert not torch.equal(refs[0], refs[1])
        assert not torch.equal(fitness[0], fitness[1])

    # 7. validation
    def test_validation_raises_before_launch(self, monkeypatch):
        dev = _dev()
        pop_in = _population(3, dev)
        thetas, obs_mu, obs_nu, env_A, env_B = pop_in
        seeds = ops.pair_seeds(SEEDS[:3], dev)
        fitness = torch.rand(3, 8, device=dev)
        wpair = torch.rand(3, 4, device=dev)
        real = ops._OPS
        launches = []

        class Recorder:
            es_grad_chunks = staticmethod(real.es_grad_chunks)

            def es_rollout_mlp_pairs(self, *args):
                launches.append(("rollout", args))

            def centered_rank_pairs(self, *args):
                launches.append(("rank", args))

            def es_grad_pairs(self, *args):
                launches.append(("grad", args))

        monkeypatch.setattr(ops, "_OPS", Recorder())

        def rollout(horizon=8, pop=8, **kw):
            a = dict(thetas=thetas, seeds=seeds, obs_mu=obs_mu,
                     obs_nu=obs_nu, env_A=env_A, env_B=env_B)
            a.update(kw)
            return ops.es_rollout_mlp_pairs(
                a["thetas"], SIGMA, a["seeds"], ITER, horizon, pop,
                a["obs_mu"], a["obs_nu"], a["env_A"], a["env_B"])

        # wrong dtype
        with pytest.raises(TypeError):
            rollout(thetas=thetas.double())
        with pytest.raises(TypeError):
            rollout(seeds=seeds.long())
        with pytest.raises(TypeError):
            rollout(seeds=seeds.float())
        with pytest.raises(TypeError):
            ops.centered_rank_pairs(fitness.double())
        with pytest.raises(TypeError):
            ops.es_grad_pairs(wpair.half(), seeds, ITER)
        with pytest.raises(TypeError):
            ops.es_grad_pairs(wpair, seeds.long(), ITER)
        # CPU tensor
        with pytest.raises(TypeError):
            rollout(obs_nu=obs_nu.cpu())
        with pytest.raises(TypeError):
            rollout(seeds=seeds.cpu())
        with pytest.raises(TypeError):
            ops.centered_rank_pairs(fitness.cpu())
        with pytest.raises(TypeError):
            ops.es_grad_pairs(wpair, seeds.cpu(), ITER)
        # non-contiguous
        wide = torch.zeros(3, 2 * ops.NPARAMS, device=dev)
        assert wide[:, ::2].shape == thetas.shape
        with pytest.raises(TypeError):
            rollout(thetas=wide[:, ::2])
        with pytest.raises(TypeError):
            ops.centered_rank_pairs(torch.rand(3, 16, device=dev)[:, ::2])
        with pytest.raises(TypeError):
            ops.es_grad_pairs(torch.rand(3, 8, device=dev)[:, ::2], seeds,
                              ITER)
        # odd pop, horizon 0
        with pytest.raises(ValueError):
            rollout(pop=7)
        with pytest.raises(ValueError):
            rollout(horizon=0)
        # mismatched P and other shapes
        with pytest.raises(ValueError):
            rollout(obs_mu=obs_mu[:2].contiguous())
        with pytest.raises(ValueError):
            rollout(seeds=seeds[:2].contiguous())
        with pytest.raises(ValueError):
            rollout(env_A=torch.cat([env_A, env_A]))
        with pytest.raises(ValueError):
            rollout(env_B=env_B[:, :3].contiguous())
        with pytest.raises(ValueError):
            rollout(thetas=thetas[:, :-1].contiguous())
        with pytest.raises(ValueError):
            ops.es_grad_pairs(wpair, seeds[:2].contiguous(), ITER)
        with pytest.raises(ValueError):
            ops.es_grad_pairs(wpair[0], seeds, ITER)
        with pytest.raises(ValueError):
            ops.centered_rank_pairs(fitness[0])
        # the launch grid
        with pytest.raises(ValueError):
            rollout(pop=2 ** 30)
        # n > 16384
        with pytest.raises(ValueError):
            ops.centered_rank_pairs(torch.zeros(1, 16385, device=dev))
        assert launches == []
        # the recorder does see valid calls: the checks above are live
        rollout()
        ops.centered_rank_pairs(fitness)
        ops.centered_rank_pairs(torch.zeros(1, 16384, device=dev))
        ops.es_grad_pairs(wpair, seeds, ITER)
        assert [name for name, _ in launches] == ["rollout", "rank", "rank",
                                                  "grad"]

    def test_failed_validation_leaves_outputs_alone(self):
        """With the real extension: a rejected call between two valid ones
        changes nothing that they return."""
        pop_in = _population(3, _dev())
        seeds = SEEDS[:3]
        fit1, stat1 = _run_pairs(pop_in, seeds, 8, 8)
        keep_f, keep_s = fit1.clone(), stat1.clone()
        with pytest.raises(ValueError):
            _run_pairs(pop_in, seeds, 0, 8)
        with pytest.raises(ValueError):
            _run_pairs(pop_in, seeds, 8, 7)
        torch.cuda.synchronize()
        assert _same_bits(fit1, keep_f) and _same_bits(stat1, keep_s)
        fit2, stat2 = _run_pairs(pop_in, seeds, 8, 8)
        assert _same_bits(fit2, keep_f) and _same_bits(stat2, keep_s)

    def test_pair_seeds_masks_like_the_scalar_ops(self):
        sd = ops.pair_seeds([1, 1 << 31, (1 << 32) + 5, -1], "cpu")
        assert sd.dtype == torch.int32 and sd.is_contiguous()
        assert sd.tolist() == [1, -(1 << 31), 5, -1]


# 6. population vs engines, bit
_ENGINE_FIELDS = ("theta", "adam_m", "adam_v", "obs_sum", "obs_sumsq",
                  "obs_count", "obs_mu", "obs_nu")


def _assert_population_equals_engines(pop, engines, what):
    for p, eng in enumerate(engines):
        for f in _ENGINE_FIELDS:
            got = getattr(pop, f)[p]
            want = getattr(eng, f)
            assert _same_bits(got, want), (what, p, f, got, want)
        assert pop.t_step == eng.t_step


@requires_gpu
class TestESPopulation:
    def _build(self):
        dev = _dev()
        cfg = ESConfig(pop_per_gpu=64, horizon=8)
        seeds = SEEDS[:3]
        envs = [es_engine.make_env_params(200 + p, "cpu") for p in range(3)]
        pop = ESPopulation(cfg, seeds, envs, device=dev)
        engines = [ESEngine(dataclasses.replace(cfg, seed=seeds[p]),
                            ctx=None, device=dev, env_params=envs[p])
                   for p in range(3)]
        return cfg, seeds, envs, pop, engines

    def test_population_matches_engines(self):
        cfg, seeds, envs, pop, engines = self._build()
        dev = pop.device
        assert len(pop) == 3
        _assert_population_equals_engines(pop, engines, "init")
        for it in range(3):
            stats = pop.step()
            for eng in engines:
                eng.step()
            _assert_population_equals_engines(pop, engines, "step %d" % it)
        for key in ("fitness_mean", "fitness_max", "grad_norm"):
            assert stats[key].shape == (3,) and stats[key].is_cuda, key
        assert stats["rollouts"] == 3 * 64 * 64
        # the pairs really are different problems
        assert pop.theta.unique(dim=0).shape[0] == 3
        assert pop.obs_sum.unique(dim=0).shape[0] == 3
        assert stats["fitness_mean"].unique().numel() == 3

        # transfer matrix: the stacked state, no gather
        scores = pop.transfer_matrix(8, 1234, ITER)
        want = transfer_matrix(engines, 8, 1234, ITER)
        assert scores.shape == (3, 3) and _same_bits(scores, want)
        assert scores.flatten().unique().numel() == 9

        # a chain: donors are read from the pre-transfer state
        moves = [(0, 1), (1, 2)]
        env_before = pop.env_A.clone()
        pop.apply_transfers(moves)
        apply_transfers(engines, moves)
        _assert_population_equals_engines(pop, engines, "transfers")
        assert not pop.adam_m[0].any() and not pop.adam_v[1].any()
        assert pop.adam_m[2].any()
        assert not torch.equal(pop.theta[0], pop.theta[1])
        assert torch.equal(pop.env_A, env_before)

        # a pair lifted out into a plain engine takes engine p's next step
        for p in range(3):
            fresh = ESEngine(dataclasses.replace(cfg, seed=seeds[p]),
                             ctx=None, device=dev, env_params=envs[p])
            fresh.load_state_dict(pop.engine_state(p))
            s_fresh, s_eng = fresh.step(), engines[p].step()
            assert s_fresh == s_eng, p
            for f in _ENGINE_FIELDS:
                assert _same_bits(getattr(fresh, f),
                                  getattr(engines[p], f)), (p, f)
        # ... and the population takes the same step
        pop.step()
        _assert_population_equals_engines(pop, engines, "after transfers")

    def test_set_env_and_state_dict_round_trip(self):
        cfg, seeds, envs, pop, engines = self._build()
        pop.step()
        new_A, new_B = es_engine.make_env_params(999, "cpu")
        pop.set_env(1, new_A, new_B)
        engines[1].step()
        engines[1].env_A.copy_(new_A)
        engines[1].env_B.copy_(new_B)
        assert torch.equal(pop.env_A[1].cpu(), new_A)
        assert torch.equal(pop.env_A[0].cpu(), envs[0][0])
        with pytest.raises(ValueError):
            pop.set_env(0, new_A[:3], new_B)

        state = pop.state_dict()
        twin = ESPopulation(cfg, seeds, envs, device=pop.device)
        twin.load_state_dict(state)
        pop.step()
        twin.step()
        engines[1].step()
        for f in _ENGINE_FIELDS + ("env_A", "env_B"):
            assert _same_bits(getattr(pop, f), getattr(twin, f)), f
        assert twin.t_step == pop.t_step == 2
        for f in _ENGINE_FIELDS:
            assert _same_bits(getattr(pop, f)[1], getattr(engines[1], f)), f
        other = ESPopulation(cfg, seeds[::-1], envs, device=pop.device)
        with pytest.raises(ValueError):
            other.load_state_dict(state)


# 8. example
@requires_gpu
def test_example_batched_prints_the_same_generations():
    def run(*extra):
        proc = subprocess.run(
            [sys.executable, os.path.join(REPO, "examples",
                                          "poet_transfer.py"),
             "--pairs", "3", "--generations", "2", "--pop", "64",
             "--horizon", "8", "--inner-steps", "1"] + list(extra),
            capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stdout + proc.stderr
        return [ln for ln in proc.stdout.splitlines()
                if ln.startswith("gen ")]

    plain, batched = run(), run("--batched")
    assert len(plain) == 2, plain
    assert batched == plain, (plain, batched)
