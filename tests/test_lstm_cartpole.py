"""What tests/gpu/test_lstm_cartpole_gpu.py needs settled without a GPU: the
inputs it runs leave few steps undecided, and the wrapper refuses a bad call
before any launch."""

import numpy as np
import pytest
import torch

import cartpole_cases as K
from fiber_amd import ops
from fiber_amd.es import cartpole_oracle as C
from fiber_amd.es import init_theta_lstm
from fiber_amd.es import lstm_cartpole_oracle as LC

MASKS = (0b0101, 0b1111)


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("sigma", K.SIGMAS)
@pytest.mark.parametrize("cart", list(K.CARTS))
def test_gpu_inputs_are_mostly_decided(cart, sigma, mask):
    """The two oracles chained for 60 steps on the GPU test's inputs: at
    most 1 % of the live environment-steps are undecided, well inside the
    5 % the GPU test allows."""
    theta = init_theta_lstm(K.SEED, "cpu").numpy()
    s0 = C.init_states(K.SEED, K.ITER)[0]
    undecided = live = 0
    for m in range(K.POP):
        pol = LC.member_policy(theta, sigma, K.SEED, K.ITER, K.OFFSET + m)
        u, n = LC.undecided_share(pol, K.MU, K.NU, mask, K.CARTS[cart], s0,
                                  60)
        undecided, live = undecided + u, live + n
    print("%s mask %s sigma %g: %d of %d undecided"
          % (cart, format(mask, "04b"), sigma, undecided, live))
    assert 0 < live < 64 * K.POP * 60     # episodes end inside the chain
    assert undecided <= 0.01 * live


def test_wrapper_refuses_before_launching():
    theta = init_theta_lstm(K.SEED, "cpu")
    mu, nu = torch.from_numpy(K.MU), torch.from_numpy(K.NU)
    cart = ops.cartpole_params()
    with pytest.raises(TypeError, match="float32"):
        ops.es_rollout_lstm_cartpole(theta.double(), 0.05, 1, 0, 4, 0, 2, mu,
                                     nu, cart)
    with pytest.raises(TypeError, match="CUDA"):   # not on the GPU
        ops.es_rollout_lstm_cartpole(theta, 0.05, 1, 0, 4, 0, 2, mu, nu, cart)
