"""Fixed inputs of the wide-policy rollout step test.  tests/test_wide_oracle.py
asserts from the oracle alone that at most CLOSE_CAP of their (member, env)
cases are undecided; tests/gpu/test_wide_gpu.py runs them on the kernel."""

import numpy as np
import torch

from fiber_amd.es import init_theta_wide, philox_ref
from fiber_amd.es import wide_oracle as W
from fiber_amd.es.engine import make_env_params

SEED, ITER = 4321, 3
OFFSET, POP = 2, 6
MEMBERS = (0, 1, POP - 1)   # both signs of a pair, and the last block
HORIZONS = (0, 1, 2, 7)
SIGMAS = (0.0, 0.05)
HIDDEN = (128, 256)
CLOSE_CAP = 0.05
MU = (0.05, -0.1, 0.02, 0.0)
NU = (0.3, 0.5, 0.2, 0.4)


def world(hidden, device):
    """(theta, obs_mu, obs_nu, env_A, env_B) on ``device``."""
    env_A, env_B = make_env_params(SEED, device)
    return (init_theta_wide(SEED, hidden, device),
            torch.tensor(MU, device=device), torch.tensor(NU, device=device),
            env_A, env_B)


def member_policy(theta, hidden, sigma, m):
    """Oracle policy of shard member ``m`` (numpy ``theta``)."""
    member = OFFSET + m
    z = philox_ref.noise_for_pair(SEED, ITER, member // 2,
                                  W.wide_nparams(hidden))
    return W.make_policy(theta, hidden, -sigma if member % 2 else sigma, z)


def init_state():
    return philox_ref.env_init_state(SEED, ITER, 64).astype(np.float32)
