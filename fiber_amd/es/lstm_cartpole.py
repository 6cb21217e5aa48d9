"""OpenAI-ES with the LSTM policy on CartPole (single GPU).

``CartPoleESEngine``'s environment under ``LSTMESEngine``'s policy, rolled
out by ``es_rollout_lstm_cartpole``.  ``obs_mask`` hides state dims from the
policy; the default ``0b0101`` shows the cart's position and the pole's angle
and hides both velocities, the pole-balancing task that a policy can only
solve with memory.  With ``0b1111`` it is CartPole as ``CartPoleESEngine``
runs it, under a recurrent policy.

The policy, its theta layout (``ops.LSTM_NPARAMS``) and its noise are
``LSTMESEngine``'s, so ranking, gradient and Adam are too; the hidden and the
cell state start at zero in every episode.  The environment, its start
states and the fitness (mean episode length) are ``CartPoleESEngine``'s.

Limits: hidden width 64, one cell, one GPU; there is no GRU, POET /
``ESPopulation``, novelty or GA variant of this pairing.
"""

import dataclasses

import torch

from .. import ops
from . import _core
from .cartpole import CartPoleESEngine
from .lstm import init_theta_lstm


class LSTMCartPoleESEngine(_core.RolloutESEngine):
    nparams = ops.LSTM_NPARAMS
    _range = "es.rollout_lstm_cartpole"

    def __init__(self, config, ctx=None, device=None, env_params=None,
                 obs_mask=0b0101):
        """``env_params``: a ``cart[8]`` tensor, None for Gym's values, as
        in ``CartPoleESEngine``, and like it not part of ``state_dict()``;
        ``obs_mask`` is, as in ``RecurrentESEngine``."""
        if ctx is not None:
            raise NotImplementedError(
                "LSTMCartPoleESEngine is single-GPU: no ring context")
        obs_mask = int(obs_mask)
        if not 0 <= obs_mask < 2 ** config.obs_dim:
            raise ValueError("obs_mask must be in [0, %d), got %d"
                             % (2 ** config.obs_dim, obs_mask))
        self.obs_mask = obs_mask
        super().__init__(config, device, env_params)

    def _init_theta(self):
        return init_theta_lstm(self.cfg.seed, self.device)

    _resolve_env = CartPoleESEngine._resolve_env

    def _rollout(self, sigma, iteration, horizon, pop):
        return ops.es_rollout_lstm_cartpole(
            self.theta, sigma, self.cfg.seed, iteration, horizon, 0, pop,
            self.obs_mu, self.obs_nu, self.cart, self.obs_mask)

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

    def act(self, obs, state=None):
        """``(actions[n], (h'[n][64], c'[n][64]))`` of the current theta for
        raw states ``obs[n][4]`` and the carried ``state = (h, c)`` (None:
        zeros, the start of an episode), as ``LSTMESEngine.act``: normalised,
        masked by ``obs_mask``, through ``ops.lstm_policy_step``.  Action 0
        pushes left, 1 (``l1 > l0``) right."""
        x = _core.act_input(self, obs, self.obs_mask)
        if state is None:
            state = tuple(torch.zeros(obs.shape[0], self.cfg.hidden,
                                      device=obs.device) for _ in range(2))
        logits, hnew, cnew = ops.lstm_policy_step(self.theta, x, *state)
        return (logits[:, 1] > logits[:, 0]).to(torch.int64), (hnew, cnew)

    def state_dict(self):
        return {
            **self._state(),
            "obs_mask": self.obs_mask,
            "config": dataclasses.asdict(self.cfg),
        }

    def load_state_dict(self, state):
        self._load_state(state)
        self.obs_mask = int(state["obs_mask"])

    save, load = _core.save, _core.load
