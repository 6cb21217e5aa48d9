"""OpenAI-ES on CartPole with the 4 -> 64 -> 64 -> 2 MLP policy (single GPU).

``ESEngine``'s iteration with the rollout swapped for
``es_rollout_mlp_cartpole``: Gym CartPole-v1's physics stepped inside the
rollout kernel, episodes that end when the cart or the pole leaves its
range, and a fitness that is the mean episode length.  The policy, its theta
layout and its noise are ``ESEngine``'s, so ranking, gradient and Adam are
too.

The environment is ``cart[8]`` (``ops.cartpole_params``).  Every iteration
starts its 64 episodes per member from ``0.05 * z``, ``z`` drawn per (seed,
iteration): common random numbers across the members.

Limits: one GPU; there is no POET / ``ESPopulation``, novelty or GA variant
on this environment.  The recurrent variant is ``LSTMCartPoleESEngine``
(lstm_cartpole.py), which can also hide the velocities from the policy.
"""

import dataclasses

import torch

from .. import ops
from . import _core
from .engine import ESConfig, init_theta


class CartPoleESEngine(_core.RolloutESEngine):
    nparams = ops.NPARAMS
    _range = "es.rollout_cartpole"

    def __init__(self, config: ESConfig, ctx=None, device=None,
                 env_params=None):
        """``env_params``: a ``cart[8]`` tensor, None for Gym's values.  It
        is not part of ``state_dict()``, like the other engines'
        environments."""
        if ctx is not None:
            raise NotImplementedError(
                "CartPoleESEngine is single-GPU: no ring context")
        super().__init__(config, device, env_params)

    def _init_theta(self):
        return init_theta(self.cfg.seed, self.device)

    def _resolve_env(self, env_params):
        if env_params is None:
            self.cart = ops.cartpole_params(device=self.device)
            return
        if tuple(env_params.shape) != (ops.CART_NPARAMS,):
            raise ValueError("env_params must be cart[%d], got %s"
                             % (ops.CART_NPARAMS, tuple(env_params.shape)))
        # through cartpole_params for its checks; an own copy, so that
        # mutating the caller's tensor later does not move the environment
        self.cart = ops.cartpole_params(*env_params.tolist(),
                                        device=self.device)

    def _rollout(self, sigma, iteration, horizon, pop):
        return ops.es_rollout_mlp_cartpole(
            self.theta, sigma, self.cfg.seed, iteration, horizon, 0, pop,
            self.obs_mu, self.obs_nu, self.cart)

    def _merge_obs_stat(self, obs_stat):
        self._steps_taken = obs_stat[8]
        super()._merge_obs_stat(obs_stat)

    def step(self, iteration=None):
        """``RolloutESEngine.step``; ``fitness_mean`` is the mean episode
        length and ``env_steps`` the steps actually taken, not
        ``pop * 64 * horizon``."""
        stats = super().step(iteration)
        stats["env_steps"] = int(self._steps_taken)
        return stats

    def act(self, obs, return_logits=False):
        """Actions (0 pushes left, 1 right) of the current theta for raw
        observations ``obs[n][4]``, as ``ESEngine.act`` forms them."""
        logits = ops.mlp_policy_forward(self.theta,
                                        _core.act_input(self, obs))
        actions = (logits[:, 1] > logits[:, 0]).to(torch.int64)
        if return_logits:
            return actions, logits
        return actions

    def state_dict(self):
        return {**self._state(), "config": dataclasses.asdict(self.cfg)}

    def load_state_dict(self, state):
        self._load_state(state)

    save, load = _core.save, _core.load
