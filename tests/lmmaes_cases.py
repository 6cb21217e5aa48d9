"""Inputs shared by tests/test_lmmaes.py and tests/gpu/test_lmmaes_gpu.py."""

import numpy as np

NPARAMS = 4610
SEED, ITER, HORIZON = 2019, 5, 4
SIGMA, SCALE = 0.05, 0.8
DIRS = (0, 1, 3, 29, 32)             # J: none, one, part of a round of 8,
#                                      the paper's m, LOWRANK_DIRS_MAX
LAUNCHES = ((2, 0), (8, 6))          # (pop_shard, member_offset)


def lowrank_inputs(J):
    """``(dirs[J][n], mix[J][J])`` float32: rows of unequal scale (a factor
    16 between the smallest and the largest), a dense random lower
    triangle that no LM-MA-ES state would give."""
    rng = np.random.default_rng(100 + J)
    rows = 0.02 * 2.0 ** (np.arange(J) % 5 - 2.0)
    dirs = rng.standard_normal((J, NPARAMS)) * rows[:, None]
    mix = np.tril(rng.standard_normal((J, J))) * 0.5
    return dirs.astype(np.float32), mix.astype(np.float32)


def chain_inputs(J):
    """``(dirs, c_d, z)`` for the closed form against the chain: rows of
    different norms (1.5 to 6), rates spread over (0, 1)."""
    rng = np.random.default_rng(200 + J)
    norms = 1.5 * 2.0 ** (np.arange(J) % 3)
    dirs = rng.standard_normal((J, NPARAMS))
    dirs *= (norms / np.linalg.norm(dirs, axis=1))[:, None]
    c_d = (np.arange(J) + 0.5) / J if J else np.zeros(0)
    return (dirs.astype(np.float32), rng.permutation(c_d),
            rng.standard_normal(NPARAMS))
