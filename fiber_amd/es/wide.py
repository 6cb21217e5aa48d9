"""OpenAI-ES with a wide feed-forward policy, hidden 128 or 256 (single GPU).

``ESEngine``'s iteration with the rollout swapped for
``es_rollout_mlp_wide``: a 4 -> H -> H -> 2 tanh policy whose perturbed W2
is drawn straight into the MFMA registers of the workgroup that rolls the
member out (fiber_amd/csrc/ops/wide_kernels.hip).  Ranking, gradient and
Adam are the 64-wide engine's; ``es_grad`` regenerates the same noise with
``nparams=ops.wide_nparams(hidden)``.

theta layout (``ops.wide_nparams(H)`` = H*H + 8H + 2): ``W1[H][4]``,
``b1[H]``, ``W2[H][H]``, ``b2[H]``, ``W3[2][H]``, ``b3[2]``.

Limits: H in ``ops.WIDE_HIDDEN``, two hidden layers, one GPU; there is no
POET, ``ESPopulation``, NS-ES, SNES, GA or MAP-Elites variant.
"""

import dataclasses

import torch

from .. import ops
from . import _core
from .engine import ESConfig


def init_theta_wide(seed, hidden, device):
    """Per-layer scaled normals (fan-in ** -0.5, as ``init_theta``), zero
    biases."""
    n = ops.wide_nparams(hidden)
    H = int(hidden)
    gen = torch.Generator().manual_seed(seed)
    theta = torch.zeros(n)
    o_w2, o_w3 = 5 * H, 6 * H + H * H
    theta[:4 * H] = (torch.randn(H, 4, generator=gen) / 4 ** 0.5).reshape(-1)
    theta[o_w2:o_w2 + H * H] = (torch.randn(H, H, generator=gen)
                                / H ** 0.5).reshape(-1)
    theta[o_w3:o_w3 + 2 * H] = (torch.randn(2, H, generator=gen)
                                / H ** 0.5).reshape(-1)
    return theta.to(device).contiguous()


class WideESEngine(_core.RolloutESEngine):
    _range = "es.rollout_wide"

    def __init__(self, config: ESConfig, hidden, ctx=None, device=None,
                 env_params=None):
        if ctx is not None:
            raise NotImplementedError(
                "WideESEngine is single-GPU: no ring context")
        self.nparams = ops.wide_nparams(hidden)   # refuses 64 and the rest
        self.hidden = int(hidden)
        super().__init__(config, device, env_params)

    def _init_theta(self):
        return init_theta_wide(self.cfg.seed, self.hidden, self.device)

    def _rollout(self, sigma, iteration, horizon, pop):
        return ops.es_rollout_mlp_wide(
            self.theta, self.hidden, sigma, self.cfg.seed, iteration,
            horizon, 0, pop, self.obs_mu, self.obs_nu, self.env_A,
            self.env_B)

    # -- act with the current policy --------------------------------------
    def act(self, obs, return_logits=False):
        """Actions of the current theta for raw observations ``obs[n][4]``
        (fp32, on this engine's device): normalised as ``ESEngine.act``
        does and sent through ``ops.mlp_policy_forward_wide``.  Returns
        int64 ``actions[n]``, 1 where ``l1 > l0`` (a tie is 0), or
        ``(actions, logits)``.  The serving kernel keeps ``h2`` in fp32 as
        the step loop does, so both choose alike."""
        logits = ops.mlp_policy_forward_wide(self.theta, self.hidden,
                                             _core.act_input(self, obs))
        actions = (logits[:, 1] > logits[:, 0]).to(torch.int64)
        if return_logits:
            return actions, logits
        return actions

    # -- checkpoint / resume ----------------------------------------------
    def state_dict(self):
        return {
            **self._state(),
            "hidden": self.hidden,
            "config": dataclasses.asdict(self.cfg),
        }

    def load_state_dict(self, state):
        if int(state["hidden"]) != self.hidden:
            raise ValueError("checkpoint has hidden = %d, the engine %d"
                             % (int(state["hidden"]), self.hidden))
        self._load_state(state)

    save, load = _core.save, _core.load
