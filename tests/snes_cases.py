"""Case lists and inputs shared by tests/test_snes.py (CPU) and
tests/gpu/test_snes_gpu.py.  Everything here runs without a GPU, is computed
once per process and is never modified by a test."""

import functools

import numpy as np

import rollout_oracle_cases as RC
import update_oracle_cases as UC
from fiber_amd.es import philox_ref
from fiber_amd.es import rollout_oracle
from fiber_amd.es import snes_oracle
from fiber_amd.es import update_oracle

NP_MLP, NP_CONV = UC.NP_MLP, UC.NP_CONV

# ---- es_rollout_mlp_sigma: uniform sigma ---------------------------------
UNIFORM_SIGMAS = (0.05, 4.0)
UNIFORM_HORIZONS = (8, 17)
UNIFORM_OFFSETS = (0, 3)
UNIFORM_POP = 8
UNIFORM_SEED = RC.SEED

# ---- es_rollout_mlp_sigma: non-uniform sigma -----------------------------
# Launches of POP members (seed, member_offset, h): all POP * 64 episodes
# are decided through h steps with sigma_vector().  Found on the CPU over
# seeds 100..139 and offsets {0, 3}; the property is asserted by the tests,
# so a stale entry fails instead of comparing undecided episodes.
POP = 4
SIGMA_H_MAX = 3
SIGMA_LAUNCHES = ((109, 3, 3), (103, 0, 2), (107, 0, 2), (109, 0, 2))


@functools.lru_cache(maxsize=None)
def sigma_vector():
    """sigma[j] = 2^-(2 + (3j + j//64) % 5): five powers of two, 1/4 down to
    1/64, that vary inside every layer (and from row to row of W2), so that
    sigma[j] * z[j] is exact in fp32."""
    j = np.arange(NP_MLP, dtype=np.int64)
    s = np.ldexp(1.0, -(2 + (3 * j + j // 64) % 5)).astype(np.float32)
    s.setflags(write=False)
    return s


def sigma_member_rollout(seed, member, horizon=SIGMA_H_MAX):
    """Oracle rollout of block ``member`` of es_rollout_mlp_sigma with
    sigma_vector(): the policy is theta +- float32(sigma * z), which
    make_policy forms from sgn = +-1 and the scaled draws."""
    theta, mu, nu, A, B = RC.member_args()
    z = philox_ref.noise_for_pair(seed, RC.ITER, member // 2, NP_MLP)
    sz = (sigma_vector() * z).astype(np.float32)
    # exact: a power of two times an fp32 value far from the subnormals
    assert np.array_equal(sz.astype(np.float64),
                          sigma_vector().astype(np.float64)
                          * z.astype(np.float64))
    s0, s0_err = rollout_oracle.init_states(seed, RC.ITER)
    pol = rollout_oracle.make_policy(theta, -1.0 if member % 2 else 1.0, sz)
    return rollout_oracle.rollout(pol, mu, nu, A, B, s0, horizon, s0_err)


@functools.lru_cache(maxsize=None)
def sigma_launch(seed, offset, pop=POP):
    """Oracle rollouts, SIGMA_H_MAX steps, of the ``pop`` members of one
    launch.  Horizon h < SIGMA_H_MAX is a prefix of it."""
    return tuple(sigma_member_rollout(seed, offset + i) for i in range(pop))


# ---- es_grad_sigma ---------------------------------------------------------
GRAD_SEED, GRAD_ITER = UC.GRAD_SEED, UC.GRAD_ITER
MLP_RANGES = UC.MLP_RANGES
SHARDS, WHOLE = UC.SHARDS, UC.WHOLE
CONV_RANGE = (2, 66)           # 64 pairs at NP_CONV: the 4-chunk split


def wdiff_weights(begin, end):
    return UC.weights(begin, end)


def wsum_weights(begin, end):
    """A second weight vector for [begin, end), laid out like
    ``UC.weights``: the same length, NaN outside the range.  Its zeros are
    placed against wdiff's (+0 at begin+1, -0 at begin+4, +0 at end-1) so
    that every combination occurs: wdiff zero alone (begin+1), wsum zero
    alone (begin+2, a -0), both zero (begin+4 and end-1: the pair is
    skipped)."""
    rng = np.random.default_rng(100 * begin + end + 7919)
    w = np.full(end + 5, np.nan, dtype=np.float32)
    w[begin:end] = (rng.random(end - begin) - 0.5).astype(np.float32)
    if end - begin >= 8:
        w[begin + 2] = -0.0
        w[begin + 4] = 0.0
        w[end - 1] = -0.0
    return w


@functools.lru_cache(maxsize=None)
def sigma_grad_reference(begin, end, nparams, wbegin=None, wend=None):
    """(g_sig, tolerance, parameter indices) of es_grad_sigma over [begin,
    end) with ``wsum_weights(wbegin, wend)`` (by default of the range
    itself); at NP_CONV on UC.conv_blocks() only."""
    if wbegin is None:
        wbegin, wend = begin, end
    jb = UC.conv_blocks() if nparams == NP_CONV else None
    g, abs_sum = snes_oracle.sigma_grad_fp64(
        wsum_weights(wbegin, wend), begin, end, GRAD_SEED, GRAD_ITER,
        nparams, jb)
    pairs = end - begin
    tol = snes_oracle.sigma_grad_tol(
        abs_sum, pairs, update_oracle.grad_chunks(pairs, nparams))
    return g, tol, update_oracle.param_index(nparams, jb)


# ---- whole step --------------------------------------------------------------
STEP_ITERATIONS = UC.STEP_ITERATIONS
STEP_POPS = UC.MLP_STEP_POPS       # 64 pairs: 32 chunks; 65: empty chunks
STEP_POP = 128
STEP_HORIZON = UC.STEP_HORIZON
STEP_LR_SIGMA = 0.5
RAIL = 0.01                        # rails 1 % either side of config.sigma
