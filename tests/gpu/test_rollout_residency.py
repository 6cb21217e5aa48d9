"""The rollout kernels at full residency against the same work one block
per CU.

In es_rollout_mlp and es_eval_matrix the layer-2 B operand h1 shares the
LDS tile that W2 is staged in, and the kernels run 7 blocks per CU.  The
sharing rests on every wave having its W2 fragments in registers before
any wave writes h1; a violation would only show when blocks are packed
onto a CU and start while their neighbours are mid-loop.  tests/gpu/
test_rollout_bits.py launches 8 blocks, far from that.

Here one launch of 4096 blocks (twice 256 CUs x 8, so every CU is full
and blocks are replaced mid-run) must give, bit for bit, what the same
members give in launches of 256 blocks (at most one block per CU), and
its first 8 members must match the recorded golden.  The obs-stat sums
are not compared: their reduction order depends on the shard.
"""

import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

HERE = os.path.dirname(os.path.abspath(__file__))

POP, SHARD = 4096, 256
HORIZON, SIGMA = 3, 0.05
EVAL_K = EVAL_M = 64
EVAL_SUB = 8


def _bits_module():
    """tests/gpu/test_rollout_bits.py: its inputs and its golden."""
    spec = importlib.util.spec_from_file_location(
        "_rollout_bits_inputs", os.path.join(HERE, "test_rollout_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@requires_gpu
def test_rollout_full_residency_matches_one_block_per_cu():
    from fiber_amd import ops

    rb = _bits_module()
    thetas, obs_mu, obs_nu, env_A, env_B = rb._inputs(
        torch.device("cuda", 0))

    def run(offset, pop):
        return ops.es_rollout_mlp(thetas[0], SIGMA, rb.SEED, rb.ITER,
                                  HORIZON, offset, pop, obs_mu[0],
                                  obs_nu[0], env_A[0], env_B[0])

    fit, stat = run(0, POP)
    parts = [run(off, SHARD) for off in range(0, POP, SHARD)]
    fit, stat = fit.cpu(), stat.cpu()
    fit_parts = torch.cat([f for f, _ in parts]).cpu()
    count_parts = sum(float(s[8]) for _, s in parts)

    golden = torch.from_numpy(np.load(rb.ROLLOUT_GOLDEN))
    row = golden[rb.CASES.index((HORIZON, 0, SIGMA))]
    assert _same_bits(fit[:rb.POP], row[:rb.POP]), (fit[:rb.POP],
                                                    row[:rb.POP])

    assert torch.isfinite(fit).all()
    bad = (fit.view(torch.int32) != fit_parts.view(torch.int32)).nonzero()
    assert bad.numel() == 0, (bad.flatten()[:16], fit[bad.flatten()[:4]],
                              fit_parts[bad.flatten()[:4]])
    assert fit.unique().numel() > POP // 2  # members really differ
    assert float(stat[8]) == count_parts == float(POP * 64 * HORIZON)


@requires_gpu
def test_eval_matrix_full_residency_matches_sub_blocks():
    from fiber_amd import ops

    rb = _bits_module()
    dev = torch.device("cuda", 0)
    K, M = EVAL_K, EVAL_M

    def f32(a, *shape):
        return torch.from_numpy(a.astype(np.float32)).view(*shape).to(dev)

    thetas = torch.stack([rb._theta(1 + k) for k in range(K)]).to(dev)
    obs_mu = f32(rb._unit(K * 4, 50) * 0.4, K, 4)
    obs_nu = f32(rb._unit(K * 4, 51) + 0.9, K, 4)
    env_A = f32(rb._unit(M * 16, 52) * 1.5, M, 4, 4)
    env_B = f32(rb._unit(M * 4, 53) * 3.0, M, 4)

    scores, episodes = ops.es_eval_matrix(
        thetas, obs_mu, obs_nu, env_A, env_B, rb.SEED, rb.ITER, HORIZON,
        return_episodes=True)
    sub_scores = torch.empty_like(scores)
    sub_episodes = torch.empty_like(episodes)
    for k0 in range(0, K, EVAL_SUB):
        for m0 in range(0, M, EVAL_SUB):
            ks, ms = slice(k0, k0 + EVAL_SUB), slice(m0, m0 + EVAL_SUB)
            s, e = ops.es_eval_matrix(
                thetas[ks], obs_mu[ks], obs_nu[ks], env_A[ms], env_B[ms],
                rb.SEED, rb.ITER, HORIZON, return_episodes=True)
            sub_scores[ks, ms] = s
            sub_episodes[ks, ms] = e

    assert torch.isfinite(scores).all()
    assert _same_bits(scores.cpu(), sub_scores.cpu())
    assert _same_bits(episodes.cpu(), sub_episodes.cpu())
    assert scores.unique().numel() > K * M // 2  # cells really differ
