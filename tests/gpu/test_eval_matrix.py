"""GPU tests for es_eval_matrix (K policies x M environments in one
launch), ESEngine.evaluate / env_params and the POET transfer step."""

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
    from fiber_amd.es import (ESConfig, ESEngine, apply_transfers,
                              select_transfers, transfer_matrix)
    from fiber_amd.es import engine as es_engine

REPO = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
SEED, ITER = 1234, 5


def _population(K, M, device):
    """Distinct thetas, normalisers and envs, so that no cell equals
    another and a k/m transposition shows."""
    thetas = torch.stack([es_engine.init_theta(11 + k, "cpu")
                          for k in range(K)])
    nu_vals = [0.5, 1.0, 2.0]
    obs_nu = torch.tensor([[nu_vals[k % 3]] * 4 for k in range(K)])
    obs_mu = torch.tensor([[0.05 * (k + 1), -0.03 * k, 0.02 * k, -0.1]
                           for k in range(K)])
    envs = [es_engine.make_env_params(100 + m, "cpu") for m in range(M)]
    env_A = torch.stack([e[0] for e in envs])
    env_B = torch.stack([e[1] for e in envs])
    return [t.to(device).contiguous()
            for t in (thetas, obs_mu, obs_nu, env_A, env_B)]


def _rollout_cell(pop, k, m, horizon):
    """What the parent path computes for cell (k, m): the rollout kernel
    at sigma = 0, members 0 and 1 (+0*z and -0*z)."""
    thetas, obs_mu, obs_nu, env_A, env_B = pop
    fit, _stat = ops.es_rollout_mlp(
        thetas[k], 0.0, SEED, ITER, horizon, 0, 2, obs_mu[k], obs_nu[k],
        env_A[m], env_B[m])
    return fit


@pytest.fixture(scope="module")
def pop32():
    device = torch.device("cuda", 0)
    pop = _population(3, 2, device)
    scores, episodes = ops.es_eval_matrix(*pop, SEED, ITER, 8,
                                          return_episodes=True)
    torch.cuda.synchronize()
    return pop, scores, episodes


@requires_gpu
class TestEvalMatrixKernel:
    def test_bit_identical_to_rollout_kernel(self, pop32):
        pop, scores, _episodes = pop32
        assert scores.shape == (3, 2)
        for k in range(3):
            for m in range(2):
                fit = _rollout_cell(pop, k, m, 8)
                for member in range(2):
                    assert torch.equal(scores[k, m], fit[member]), (
                        k, m, member, scores[k, m].item(),
                        fit[member].item())
        # the cells really differ (else the identity shows nothing)
        assert scores.flatten().unique().numel() == 6

    def test_bit_identical_at_horizon_one(self):
        pop = _population(3, 2, torch.device("cuda", 0))
        scores = ops.es_eval_matrix(*pop, SEED, ITER, 1)
        for k in range(3):
            for m in range(2):
                fit = _rollout_cell(pop, k, m, 1)
                assert torch.equal(scores[k, m], fit[0]), (k, m)
                assert torch.equal(scores[k, m], fit[1]), (k, m)

    def test_bit_identical_single_cell(self):
        pop = _population(1, 1, torch.device("cuda", 0))
        scores = ops.es_eval_matrix(*pop, SEED, ITER, 8)
        assert scores.shape == (1, 1)
        fit = _rollout_cell(pop, 0, 0, 8)
        assert torch.equal(scores[0, 0], fit[0])
        assert torch.equal(scores[0, 0], fit[1])

    def test_scores_vs_fp32_oracle(self, pop32):
        pop, scores, episodes = pop32
        ref = es_engine.eval_matrix_reference(*pop, SEED, ITER, 8)
        err = (scores.cpu() - ref.mean(-1)).abs().max().item()
        print("max |scores - oracle| = %.3e" % err)
        assert err < 5e-2, (scores.cpu(), ref.mean(-1))

    def test_episodes(self, pop32):
        pop, scores, episodes = pop32
        assert episodes.shape == (3, 2, 64)
        ep = episodes.cpu().double()
        # scores = (fp32 sum of the 64 episode returns) / 64, and /64 is
        # exact; each of the 63 adds rounds by at most 2^-24 of a partial
        # sum that never exceeds sum(|episodes|)
        tol = 64 * 2.0 ** -24 * ep.abs().sum(-1)
        diff = (scores.cpu().double() * 64 - ep.sum(-1)).abs()
        print("max |64*score - sum(episodes)| = %.3e (tol min %.3e)"
              % (diff.max().item(), tol.min().item()))
        assert (diff <= tol).all(), (diff, tol)
        scores2, episodes2 = ops.es_eval_matrix(*pop, SEED, ITER, 8,
                                                return_episodes=True)
        assert torch.equal(scores, scores2)
        assert torch.equal(episodes, episodes2)

    def test_without_episodes_returns_tensor(self, pop32):
        pop, scores, _episodes = pop32
        out = ops.es_eval_matrix(*pop, SEED, ITER, 8)
        assert isinstance(out, torch.Tensor)
        assert torch.equal(out, scores)
        out = ops.es_eval_matrix(*pop, SEED, ITER, 8, return_episodes=False)
        assert isinstance(out, torch.Tensor)
        assert torch.equal(out, scores)

    def test_validation_raises_before_launch(self, pop32, monkeypatch):
        pop, _scores, _episodes = pop32
        thetas, obs_mu, obs_nu, env_A, env_B = pop
        launches = []

        class Recorder:
            def es_eval_matrix(self, *args):
                launches.append(args)

        monkeypatch.setattr(ops, "_OPS", Recorder())

        def call(horizon=8, **kw):
            a = dict(thetas=thetas, obs_mu=obs_mu, obs_nu=obs_nu,
                     env_A=env_A, env_B=env_B)
            a.update(kw)
            return ops.es_eval_matrix(a["thetas"], a["obs_mu"], a["obs_nu"],
                                      a["env_A"], a["env_B"], SEED, ITER,
                                      horizon)

        with pytest.raises(TypeError):
            call(thetas=thetas.double())
        with pytest.raises(TypeError):
            call(env_A=env_A.half())
        wide = torch.zeros(3, 2 * ops.NPARAMS, device=thetas.device)
        strided = wide[:, ::2]
        assert strided.shape == thetas.shape
        with pytest.raises(TypeError):
            call(thetas=strided)
        with pytest.raises(TypeError):
            call(obs_nu=obs_nu.cpu())
        with pytest.raises(ValueError):
            call(obs_mu=obs_mu[:2].contiguous())
        with pytest.raises(ValueError):
            call(env_B=torch.cat([env_B, env_B]))
        with pytest.raises(ValueError):
            call(thetas=thetas[:, :-1].contiguous())
        with pytest.raises(ValueError):
            call(horizon=0)
        assert launches == []
        # the recorder does see a valid call: the check above is live
        call()
        assert len(launches) == 1


@requires_gpu
class TestEngineEvaluate:
    def _engine(self, env_params=None):
        return ESEngine(ESConfig(pop_per_gpu=64, horizon=8), ctx=None,
                        device=torch.device("cuda", 0),
                        env_params=env_params)

    def test_env_params_are_used(self):
        env = es_engine.make_env_params(777, "cpu")
        eng = self._engine(env)
        assert eng.env_A.is_cuda and eng.env_A.is_contiguous()
        assert torch.equal(eng.env_A.cpu(), env[0])
        assert torch.equal(eng.env_B.cpu(), env[1])
        default = self._engine()
        want = es_engine.make_env_params(default.cfg.seed, "cpu")
        assert torch.equal(default.env_A.cpu(), want[0])
        assert torch.equal(default.env_B.cpu(), want[1])
        # a different environment gives a different score
        assert eng.evaluate().item() != default.evaluate().item()
        assert "env_A" not in eng.state_dict()

    def test_evaluate_equals_direct_call(self):
        eng = self._engine(es_engine.make_env_params(777, "cpu"))
        eng.step()  # non-trivial normaliser and t_step
        got, episodes = eng.evaluate(return_episodes=True)
        assert got.shape == () and got.is_cuda
        assert episodes.shape == (64,)
        want, want_ep = ops.es_eval_matrix(
            eng.theta[None], eng.obs_mu[None], eng.obs_nu[None],
            eng.env_A[None], eng.env_B[None], eng.cfg.seed, eng.t_step,
            eng.cfg.horizon, return_episodes=True)
        assert torch.equal(got, want[0, 0])
        assert torch.equal(episodes, want_ep[0, 0])
        assert torch.equal(eng.evaluate(), got)
        other = eng.evaluate(horizon=3, iteration=9)
        want = ops.es_eval_matrix(
            eng.theta[None], eng.obs_mu[None], eng.obs_nu[None],
            eng.env_A[None], eng.env_B[None], eng.cfg.seed, 9, 3)
        assert torch.equal(other, want[0, 0])

    def test_evaluate_leaves_engine_untouched(self):
        env = es_engine.make_env_params(777, "cpu")
        eng, twin = self._engine(env), self._engine(env)
        eng.step()
        twin.step()
        before = {k: (v.clone() if torch.is_tensor(v) else v)
                  for k, v in eng.state_dict().items()}
        mu, nu = eng.obs_mu.clone(), eng.obs_nu.clone()
        eng.evaluate()
        eng.evaluate(return_episodes=True)
        after = eng.state_dict()
        for key, val in before.items():
            if torch.is_tensor(val):
                assert torch.equal(val, after[key]), key
            else:
                assert val == after[key], key
        assert torch.equal(mu, eng.obs_mu) and torch.equal(nu, eng.obs_nu)
        s1, s2 = eng.step(), twin.step()
        assert torch.equal(eng.theta, twin.theta)
        assert s1 == s2


@requires_gpu
class TestPoetTransfer:
    def test_transfer_matrix_and_apply(self):
        device = torch.device("cuda", 0)
        engines = []
        for i in range(3):
            cfg = ESConfig(pop_per_gpu=64, horizon=8, seed=50 + i)
            engines.append(ESEngine(
                cfg, ctx=None, device=device,
                env_params=es_engine.make_env_params(200 + i, "cpu")))
            engines[-1].step()
        scores = transfer_matrix(engines, 8, SEED, ITER)
        assert scores.shape == (3, 3)
        want = ops.es_eval_matrix(
            torch.stack([e.theta for e in engines]),
            torch.stack([e.obs_mu for e in engines]),
            torch.stack([e.obs_nu for e in engines]),
            torch.stack([e.env_A for e in engines]),
            torch.stack([e.env_B for e in engines]), SEED, ITER, 8)
        assert torch.equal(scores, want)
        # row k is policy k, column m is engine m's environment
        cell = ops.es_eval_matrix(
            engines[2].theta[None], engines[2].obs_mu[None],
            engines[2].obs_nu[None], engines[0].env_A[None],
            engines[0].env_B[None], SEED, ITER, 8)
        assert torch.equal(scores[2, 0], cell[0, 0])
        assert select_transfers(scores) == select_transfers(scores.cpu())

        donor_theta = engines[1].theta.clone()
        donor_mu = engines[1].obs_mu.clone()
        env_before = engines[0].env_A.clone()
        assert engines[0].adam_m.any()
        apply_transfers(engines, [(0, 1)])
        assert torch.equal(engines[0].theta, donor_theta)
        assert torch.equal(engines[0].obs_mu, donor_mu)
        assert torch.equal(engines[0].obs_sum, engines[1].obs_sum)
        assert not engines[0].adam_m.any()
        assert not engines[0].adam_v.any()
        assert torch.equal(engines[0].env_A, env_before)
        assert torch.equal(engines[1].theta, donor_theta)
        # the receiver trains on from the donor's policy
        engines[0].step()
        assert not torch.equal(engines[0].theta, donor_theta)

    def test_example_runs(self):
        proc = subprocess.run(
            [sys.executable, os.path.join(REPO, "examples",
                                          "poet_transfer.py"),
             "--pairs", "3", "--generations", "2", "--pop", "64",
             "--horizon", "8", "--inner-steps", "1"],
            capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stdout + proc.stderr
        assert proc.stdout.count("transfers=") == 2, proc.stdout
