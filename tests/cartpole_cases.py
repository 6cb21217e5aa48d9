"""The inputs that tests/test_cartpole_oracle.py conditions on the CPU and
tests/gpu/test_cartpole_gpu.py runs on the GPU."""

import numpy as np

from fiber_amd.es import cartpole_oracle as C
from fiber_amd.es.engine import init_theta

SEED, ITER = 4321, 3
OFFSET, POP = 2, 6
SIGMAS = (0.0, 0.05)
MU = np.array([0.01, -0.05, 0.005, 0.02], dtype=np.float32)
NU = np.array([0.02, 0.3, 0.02, 0.4], dtype=np.float32)
CARTS = {
    "default": C.cart_array(),
    # every entry changed: a small x_threshold, a short pole, a weak push
    "small": C.cart_array(9.81, 0.8, 0.2, 0.25, 5.0, 0.025, 0.1, 0.15),
}
# (cart, iteration) of two-member launches, sigma 0.05 and STAT_H steps, in
# which the oracle decides every step of all 128 environments: found by
# trying iterations 0 .. 59 on the CPU
STAT_H = 12
STAT_ITERS = {"small": 8, "default": 45}


def theta():
    return init_theta(SEED, "cpu").numpy()


def members(sigma, cart, horizon, iteration=ITER, pop=POP):
    """The oracle's chained rollouts of the tested members."""
    th = theta()
    return [C.member_rollout(th, sigma, SEED, iteration, horizon, OFFSET + m,
                             MU, NU, CARTS[cart]) for m in range(pop)]
