"""OpenAI-ES with a GRU recurrent policy (single GPU).

``ESEngine``'s iteration with the rollout swapped for ``es_rollout_gru``:
a gated cell 4 -> 64 -> 2 in torch.nn.GRUCell's convention whose hidden
state starts at zero in every episode and is carried in fp32 registers for
the whole horizon.  ``obs_mask`` hides observation dims from the policy,
which is what the memory is for: with part of the state hidden a
feed-forward policy has nothing to integrate over.

theta layout (``ops.GRU_NPARAMS`` = 13442, gate order r, z, n):
``W_i[3][64][4]``, ``W_h[3][64][64]``, ``b_r b_z b_in b_hn`` (64 each; the
input and hidden biases of r and z are merged, only their sum is
identifiable), ``W_o[2][64]``, ``b_o[2]``.
"""

import dataclasses

import torch

from .. import ops
from . import _core
from .engine import ESConfig


def init_theta_gru(seed, device):
    """Per-block scaled normals (fan-in ** -0.5, as ``init_theta``), zero
    biases."""
    gen = torch.Generator().manual_seed(seed)
    theta = torch.zeros(ops.GRU_NPARAMS)
    theta[:768] = (torch.randn(3, 64, 4, generator=gen) / 4 ** 0.5).reshape(-1)
    theta[768:13056] = (torch.randn(3, 64, 64, generator=gen)
                        / 64 ** 0.5).reshape(-1)
    theta[13312:13440] = (torch.randn(2, 64, generator=gen)
                          / 64 ** 0.5).reshape(-1)
    return theta.to(device).contiguous()


class RecurrentESEngine(_core.RolloutESEngine):
    nparams = ops.GRU_NPARAMS
    _range = "es.rollout_gru"

    def __init__(self, config: ESConfig, ctx=None, device=None,
                 env_params=None, obs_mask=0b1111):
        if ctx is not None:
            raise NotImplementedError(
                "RecurrentESEngine is single-GPU: no ring context")
        super().__init__(config, device, env_params)
        if not 0 <= int(obs_mask) < 2 ** config.obs_dim:
            raise ValueError("obs_mask must be in [0, %d), got %r"
                             % (2 ** config.obs_dim, obs_mask))
        self.obs_mask = int(obs_mask)

    def _init_theta(self):
        return init_theta_gru(self.cfg.seed, self.device)

    def _rollout(self, sigma, iteration, horizon, pop):
        return ops.es_rollout_gru(
            self.theta, sigma, self.cfg.seed, iteration, horizon, 0, pop,
            self.obs_mu, self.obs_nu, self.env_A, self.env_B, self.obs_mask)

    # -- act with the current policy --------------------------------------
    def act(self, obs, hidden=None):
        """``(actions[n], hidden'[n][64])`` of the current theta for raw
        observations ``obs[n][4]`` and the carried ``hidden`` (None: zeros,
        the start of an episode).  The observation is normalised as
        ``ESEngine.act`` does, its hidden dims set to 0, and goes through
        ``ops.gru_policy_step``; an action is 1 where ``l1 > l0``."""
        x = _core.act_input(self, obs, self.obs_mask)
        if hidden is None:
            hidden = torch.zeros(obs.shape[0], self.cfg.hidden,
                                 device=obs.device)
        logits, hnew = ops.gru_policy_step(self.theta, x, hidden)
        return (logits[:, 1] > logits[:, 0]).to(torch.int64), hnew

    # -- checkpoint / resume ----------------------------------------------
    def state_dict(self):
        return {
            **self._state(),
            "obs_mask": self.obs_mask,
            "config": dataclasses.asdict(self.cfg),
        }

    def load_state_dict(self, state):
        self._load_state(state)
        self.obs_mask = int(state["obs_mask"])
