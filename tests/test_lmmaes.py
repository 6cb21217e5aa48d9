"""LM-MA-ES on the CPU: the closed form the kernels sample through against
the paper's chain, and the recombination weights (fiber_amd/es/lmmaes.py
against fiber_amd/es/lmmaes_oracle.py, float64)."""

import numpy as np
import pytest
import torch

import lmmaes_cases as C
from fiber_amd import ops
from fiber_amd.es import lmmaes
from fiber_amd.es import lmmaes_oracle as oracle


@pytest.mark.parametrize("J", (1, 2, 29, 32))
def test_sampling_mix_is_the_chain(J):
    dirs, c_d, z = C.chain_inputs(J)
    scale, mix = lmmaes.sampling_mix(torch.from_numpy(dirs), list(c_d))
    mix = mix.numpy()
    assert mix.dtype == np.float64 and mix.shape == (J, J)
    assert np.array_equal(mix, np.tril(mix))
    M = dirs.astype(np.float64)
    got = scale * z + M.T @ (mix @ (M @ z))
    want = oracle.transform_chain(dirs, c_d, z)
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    # the low-rank part is no rounding error of the identity part
    assert np.linalg.norm(want - scale * z) > 1e-3 * np.linalg.norm(want)


@pytest.mark.parametrize("pop", (2, 8, 30, 256))
def test_recombination_weights(pop):
    w, mu_w = lmmaes.recombination_weights(pop)
    want, want_mu_w = oracle.weights(pop)
    assert w.dtype == torch.float64
    assert abs(float(w.sum()) - 1.0) < 1e-14
    assert int((w > 0).sum()) == pop // 2
    assert bool((w[0] >= w).all()) and (pop == 2 or w[0] > w[1])
    np.testing.assert_allclose(w.numpy(), want, rtol=1e-14, atol=0)
    assert abs(mu_w - want_mu_w) <= 1e-13 * want_mu_w

    # ties, so that the fixed tie order decides positions
    fitness = torch.from_numpy(np.random.default_rng(pop).integers(
        0, pop // 2 + 1, pop).astype(np.float32))
    got = lmmaes.pair_weights(ops.centered_rank_ref(fitness), w.float())
    want_pair, tol = oracle.wpair_from_fitness(fitness.numpy())
    assert np.all(np.abs(got.double().numpy() - want_pair) <= tol)


def test_paper_constants():
    lm = lmmaes.LMMAESConfig().resolved(lmmaes.ESConfig())
    c_sigma, c_d, c_c = oracle.paper_rates(29)
    assert lm.n_dirs == oracle.default_n_dirs() == 29
    assert lm.c_sigma == c_sigma
    np.testing.assert_allclose(lm.c_d, c_d, rtol=1e-15)
    np.testing.assert_allclose(lm.c_c, c_c, rtol=1e-15)
    assert max([lm.c_sigma] + lm.c_d + lm.c_c) < 1.0
