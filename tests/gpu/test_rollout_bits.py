"""Bit-exactness of the MLP rollout step loop against recorded goldens.

es_rollout_mlp and es_eval_matrix share one step loop whose schedule is
tuned for VALU issue slots.  Every such change must keep each float
operation and its operand values, so the outputs stay bit-identical.  The
goldens under tests/golden/ were recorded on an MI355X from the build that
preceded the first issue-slot change (profiles/r04_rollout_issue_slots.md):

  rollout_bits_pop8.npy         [case][8 fitness + 9 obs_stat]
  eval_matrix_bits_k2m2_h17.npy [k][m][1 score + 64 episodes]

Cases: horizon in {1, 2, 3, 17} (both parities of the state double buffer
and the t < horizon-1 branch) x member_offset in {0, 6} x sigma in
{0.05, 4.0} (the large sigma drives activations into exp overflow and
underflow, the saturating path), all with a non-trivial obs normaliser and
non-zero biases.

The goldens come from the kernel itself, so they pin a build to its
predecessor, not to the mathematics.  What ties them to an independent
reading of the step loop is the fp64 oracle fiber_amd/es/rollout_oracle.py:
tests/test_rollout_oracle.py holds the recorded episodes of
eval_matrix_bits_k2m2_h17.npy to it (those whose 17 actions it calls
decided), and tests/gpu/test_rollout_oracle_gpu.py holds the kernels of the
current build to it, episode by episode, on inputs built like the ones
here.

Re-record (only ever from a build whose outputs are the accepted ones):

  python tests/gpu/test_rollout_bits.py --record
"""

import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
if __name__ == "__main__":
    sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

GOLDEN = os.path.join(REPO, "tests", "golden")
ROLLOUT_GOLDEN = os.path.join(GOLDEN, "rollout_bits_pop8.npy")
EVAL_GOLDEN = os.path.join(GOLDEN, "eval_matrix_bits_k2m2_h17.npy")

SEED, ITER, POP = 4321, 7, 8
HORIZONS = (1, 2, 3, 17)
OFFSETS = (0, 6)
SIGMAS = (0.05, 4.0)
CASES = [(h, off, sg) for h in HORIZONS for off in OFFSETS for sg in SIGMAS]
EVAL_K, EVAL_M, EVAL_H = 2, 2, 17


def _unit(n, salt):
    """n reproducible values in [-0.5, 0.5): an integer hash, exact in
    float64, so the inputs do not depend on any library's RNG stream."""
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) \
        % np.uint64(1 << 32)
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) \
        % np.uint64(1 << 32)
    h = h ^ (h >> np.uint64(13))
    return h.astype(np.float64) / float(1 << 32) - 0.5


def _theta(salt):
    """Weights at the init scale of the engine, biases non-zero."""
    from fiber_amd import ops

    th = np.zeros(ops.NPARAMS, dtype=np.float64)
    u = _unit(ops.NPARAMS, salt)
    th[:256] = u[:256] * 1.7          # W1  ~ N(0, 1/4) spread
    th[256:320] = u[256:320] * 0.6    # b1
    th[320:4416] = u[320:4416] * 0.43  # W2 ~ N(0, 1/64) spread
    th[4416:4480] = u[4416:4480] * 0.6  # b2
    th[4480:4608] = u[4480:4608] * 0.43  # W3
    th[4608:4610] = u[4608:4610] * 0.2  # b3
    return torch.from_numpy(th.astype(np.float32))


def _inputs(device):
    thetas = torch.stack([_theta(1 + k) for k in range(EVAL_K)])
    obs_mu = torch.from_numpy(
        (_unit(EVAL_K * 4, 50) * 0.4).astype(np.float32)).view(EVAL_K, 4)
    obs_nu = torch.from_numpy(
        (_unit(EVAL_K * 4, 51) + 0.9).astype(np.float32)).view(EVAL_K, 4)
    env_A = torch.from_numpy(
        (_unit(EVAL_M * 16, 52) * 1.5).astype(np.float32)).view(EVAL_M, 4, 4)
    env_B = torch.from_numpy(
        (_unit(EVAL_M * 4, 53) * 3.0).astype(np.float32)).view(EVAL_M, 4)
    return [t.to(device).contiguous()
            for t in (thetas, obs_mu, obs_nu, env_A, env_B)]


def _run_rollout(inp, horizon, offset, sigma):
    from fiber_amd import ops

    thetas, obs_mu, obs_nu, env_A, env_B = inp
    fit, stat = ops.es_rollout_mlp(thetas[0], sigma, SEED, ITER, horizon,
                                   offset, POP, obs_mu[0], obs_nu[0],
                                   env_A[0], env_B[0])
    return torch.cat([fit, stat]).cpu()


def _run_eval(inp):
    from fiber_amd import ops

    scores, episodes = ops.es_eval_matrix(*inp, SEED, ITER, EVAL_H,
                                          return_episodes=True)
    return torch.cat([scores.unsqueeze(-1), episodes], dim=-1).cpu()


@pytest.fixture(scope="module")
def inputs():
    return _inputs(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def rollout_golden():
    g = np.load(ROLLOUT_GOLDEN)
    assert g.dtype == np.float32 and g.shape == (len(CASES), POP + 9)
    return torch.from_numpy(g)


@requires_gpu
@pytest.mark.parametrize("case", range(len(CASES)),
                         ids=["h%d-off%d-sigma%g" % c for c in CASES])
def test_rollout_bits(inputs, rollout_golden, case):
    horizon, offset, sigma = CASES[case]
    got = _run_rollout(inputs, horizon, offset, sigma)
    want = rollout_golden[case]
    assert torch.isfinite(want).all()
    # bit compare: torch.equal on the int32 view also tells -0.0 from 0.0
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (
        CASES[case], got, want)
    assert torch.equal(got, want)


@requires_gpu
def test_rollout_cases_differ(rollout_golden):
    """The goldens are not degenerate: every case has its own fitness
    vector, and the members inside one case differ."""
    fits = {tuple(row[:POP].tolist()) for row in rollout_golden}
    assert len(fits) == len(CASES)
    for row in rollout_golden:
        assert row[:POP].unique().numel() == POP


@requires_gpu
def test_eval_matrix_bits(inputs):
    g = np.load(EVAL_GOLDEN)
    assert g.dtype == np.float32 and g.shape == (EVAL_K, EVAL_M, 65)
    want = torch.from_numpy(g)
    got = _run_eval(inputs)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got, want)
    assert want[..., 0].flatten().unique().numel() == EVAL_K * EVAL_M


def _record():
    assert torch.cuda.is_available(), "recording needs an MI355X"
    inp = _inputs(torch.device("cuda", 0))
    rows = torch.stack([_run_rollout(inp, *c) for c in CASES])
    ev = _run_eval(inp)
    # twice, to refuse recording anything that is not reproducible
    rows2 = torch.stack([_run_rollout(inp, *c) for c in CASES])
    assert torch.equal(rows, rows2) and torch.equal(ev, _run_eval(inp))
    os.makedirs(GOLDEN, exist_ok=True)
    np.save(ROLLOUT_GOLDEN, rows.numpy())
    np.save(EVAL_GOLDEN, ev.numpy())
    print("recorded", ROLLOUT_GOLDEN, tuple(rows.shape))
    print("recorded", EVAL_GOLDEN, tuple(ev.shape))
    print(rows[:, :POP])


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        raise SystemExit("usage: python tests/gpu/test_rollout_bits.py "
                         "--record")
    _record()
