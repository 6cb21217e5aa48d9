"""Host tests for the policy x environment evaluation: the fp32 CPU oracle,
the unchanged rollout oracle, and the POET transfer decision."""

import os
import types

import numpy as np
import torch

from fiber_amd.es import engine as es_engine
from fiber_amd.es import poet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _two_by_two():
    thetas = torch.stack([es_engine.init_theta(1, "cpu"),
                          es_engine.init_theta(2, "cpu")])
    envs = [es_engine.make_env_params(5, "cpu"),
            es_engine.make_env_params(6, "cpu")]
    env_A = torch.stack([e[0] for e in envs])
    env_B = torch.stack([e[1] for e in envs])
    obs_mu = torch.tensor([[0.0, 0.1, -0.1, 0.2], [0.05, 0.0, 0.0, -0.2]])
    obs_nu = torch.tensor([[0.5] * 4, [2.0] * 4])
    return thetas, obs_mu, obs_nu, env_A, env_B


def test_oracle_matches_rollout_reference_at_sigma_zero():
    thetas, obs_mu, obs_nu, env_A, env_B = _two_by_two()
    seed, it, horizon = 7, 3, 8
    episodes = es_engine.eval_matrix_reference(
        thetas, obs_mu, obs_nu, env_A, env_B, seed, it, horizon)
    assert episodes.shape == (2, 2, 64)
    assert episodes.dtype == torch.float32
    scores = episodes.mean(-1)
    seen = set()
    for k in range(2):
        for m in range(2):
            want = es_engine.rollout_reference(
                thetas[k], 0.0, seed, it, horizon, [0], obs_mu[k],
                obs_nu[k], env_A[m], env_B[m])[0]
            assert scores[k, m] == want, (k, m, scores[k, m], want)
            seen.add(float(want))
    # distinct policies and envs: a k/m mix-up cannot pass by accident
    assert len(seen) == 4


def test_rollout_reference_still_returns_committed_fixture():
    """The fixture was written by rollout_reference before its step body
    moved into the helper it now shares with eval_matrix_reference."""
    theta = es_engine.init_theta(42, "cpu")
    env_A, env_B = es_engine.make_env_params(42, "cpu")
    got = es_engine.rollout_reference(
        theta, 0.05, 1234, 0, 8, [0, 1, 2, 3], torch.zeros(4),
        torch.ones(4), env_A, env_B)
    want = np.load(os.path.join(GOLDEN, "rollout_reference_h8_m0to3.npy"))
    assert want.dtype == np.float32 and want.shape == (4,)
    assert np.array_equal(got.numpy(), want), (got, want)


def test_select_transfers_strict_winner():
    scores = torch.tensor([[1.0, 5.0, 0.0],
                           [0.0, 2.0, 0.0],
                           [3.0, 1.0, 4.0]])
    # column 0: row 2 (3 > 1); column 1: row 0 (5 > 2); column 2: own
    assert poet.select_transfers(scores) == [(0, 2), (1, 0)]


def test_select_transfers_exact_tie_goes_to_lowest_k():
    scores = torch.tensor([[1.0, 7.0, 7.0],
                           [0.0, 2.0, 0.0],
                           [0.0, 7.0, 7.0]])
    # column 1: rows 0 and 2 tie at 7 -> row 0; column 2: rows 0 and 2
    # tie at 7 -> row 0, which is not the incumbent (2) but does not beat
    # it either (7 > 7 is false)
    assert poet.select_transfers(scores) == [(1, 0)]


def test_select_transfers_ignores_nan_in_winning_position():
    nan = float("nan")
    scores = torch.tensor([[1.0, nan, 0.0],
                           [0.0, 2.0, 0.0],
                           [0.0, 3.0, nan]])
    # column 1: the NaN of row 0 is skipped, row 2 wins with 3 > 2;
    # column 2: the incumbent itself is NaN, so the best real score takes
    # over (rows 0 and 1 tie at 0 -> row 0)
    assert poet.select_transfers(scores) == [(1, 2), (2, 0)]
    all_nan = torch.full((3, 3), nan)
    assert poet.select_transfers(all_nan) == []


def test_select_transfers_margin():
    scores = torch.tensor([[1.0, 2.5, 0.0],
                           [1.5, 2.0, 0.0],
                           [0.0, 0.0, 1.0]])
    assert poet.select_transfers(scores) == [(0, 1), (1, 0)]
    assert poet.select_transfers(scores, margin=0.5) == []
    assert poet.select_transfers(scores, margin=0.25) == [(0, 1), (1, 0)]
    assert poet.select_transfers(scores, margin=-10.0) == [(0, 1), (1, 0)]


def test_select_transfers_best_diagonal_gives_empty_list():
    scores = torch.tensor([[3.0, 0.0, 1.0],
                           [2.0, 4.0, 1.0],
                           [1.0, 3.0, 5.0]])
    assert poet.select_transfers(scores) == []
    assert poet.select_transfers(scores.double()) == []


def _stub_engine(tag):
    """An object with the tensor attributes of ESEngine that the transfer
    touches, filled with values that identify it."""
    return types.SimpleNamespace(
        theta=torch.full((16,), float(tag)),
        adam_m=torch.full((16,), 0.5 + tag),
        adam_v=torch.full((16,), 0.25 + tag),
        obs_sum=torch.full((4,), 10.0 * tag),
        obs_sumsq=torch.full((4,), 100.0 * tag),
        obs_count=torch.full((1,), 1000.0 * tag),
        obs_mu=torch.full((4,), 0.1 * tag),
        obs_nu=torch.full((4,), 1.0 + tag),
        env_A=torch.full((4, 4), float(tag)),
        t_step=tag,
    )


def test_apply_transfers_is_order_independent():
    # a chain: 0 takes 1's policy, 1 takes 2's, 2 takes 0's
    transfers = [(0, 1), (1, 2), (2, 0)]
    results = []
    for order in (transfers, transfers[::-1],
                  [transfers[1], transfers[2], transfers[0]]):
        engines = [_stub_engine(t) for t in (1, 2, 3)]
        poet.apply_transfers(engines, order)
        results.append(engines)
    for engines in results:
        for m, k in transfers:
            donor = _stub_engine(k + 1)  # pre-transfer state of engine k
            got = engines[m]
            for f in ("theta", "obs_sum", "obs_sumsq", "obs_count",
                      "obs_mu", "obs_nu"):
                assert torch.equal(getattr(got, f), getattr(donor, f)), f
            assert not got.adam_m.any() and not got.adam_v.any()
            # the environment and the step counter stay with the pair
            assert torch.equal(got.env_A, _stub_engine(m + 1).env_A)
            assert got.t_step == m + 1


def test_apply_transfers_leaves_others_alone():
    engines = [_stub_engine(t) for t in (1, 2, 3)]
    poet.apply_transfers(engines, [(0, 2)])
    assert torch.equal(engines[0].theta, _stub_engine(3).theta)
    for i in (1, 2):
        want = _stub_engine(i + 1)
        assert torch.equal(engines[i].theta, want.theta)
        assert torch.equal(engines[i].adam_m, want.adam_m)
    # the copy does not alias the donor
    engines[2].theta.add_(1.0)
    assert torch.equal(engines[0].theta, _stub_engine(3).theta)
