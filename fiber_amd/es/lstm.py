"""OpenAI-ES with an LSTM recurrent policy (single GPU).

``RecurrentESEngine``'s iteration with the rollout swapped for
``es_rollout_lstm``: a gated cell 4 -> 64 -> 2 in torch.nn.LSTMCell's
convention whose hidden and cell state start at zero in every episode.  The
cell state is carried in fp32 registers for the whole horizon; the hidden
state is only read back through the matmul.  ``obs_mask`` hides observation
dims from the policy, as in ``RecurrentESEngine``.

theta layout (``ops.LSTM_NPARAMS`` = 17794, gate order i, f, g, o):
``W_i[4][64][4]`` at 0, ``W_h[4][64][64]`` at 1024, ``b[4][64]`` at 17408
(torch's input and hidden biases merged, only their sum is identifiable),
``W_out[2][64]`` at 17664, ``b_out[2]`` at 17792.
"""

import torch

from .. import ops
from . import _core
from .recurrent import RecurrentESEngine


def init_theta_lstm(seed, device):
    """Per-block scaled normals (fan-in ** -0.5, as ``init_theta``); zero
    biases, except the forget gate's, which is 1."""
    gen = torch.Generator().manual_seed(seed)
    theta = torch.zeros(ops.LSTM_NPARAMS)
    theta[:1024] = (torch.randn(4, 64, 4, generator=gen)
                    / 4 ** 0.5).reshape(-1)
    theta[1024:17408] = (torch.randn(4, 64, 64, generator=gen)
                         / 64 ** 0.5).reshape(-1)
    theta[17408 + 64:17408 + 128] = 1.0
    theta[17664:17792] = (torch.randn(2, 64, generator=gen)
                          / 64 ** 0.5).reshape(-1)
    return theta.to(device).contiguous()


class LSTMESEngine(RecurrentESEngine):
    """``RecurrentESEngine``'s surface (``step``, ``evaluate``,
    ``state_dict`` / ``load_state_dict``) and ``save`` / ``load`` on the LSTM
    kernels; ``act`` carries the pair ``(h, c)``."""

    nparams = ops.LSTM_NPARAMS
    _range = "es.rollout_lstm"

    def __init__(self, config, ctx=None, device=None, env_params=None,
                 obs_mask=0b1111):
        if ctx is not None:
            raise NotImplementedError(
                "LSTMESEngine is single-GPU: no ring context")
        super().__init__(config, None, device, env_params, obs_mask)

    def _init_theta(self):
        return init_theta_lstm(self.cfg.seed, self.device)

    def _rollout(self, sigma, iteration, horizon, pop):
        return ops.es_rollout_lstm(
            self.theta, sigma, self.cfg.seed, iteration, horizon, 0, pop,
            self.obs_mu, self.obs_nu, self.env_A, self.env_B, self.obs_mask)

    def act(self, obs, state=None):
        """``(actions[n], (h'[n][64], c'[n][64]))`` of the current theta for
        raw observations ``obs[n][4]`` and the carried ``state = (h, c)``
        (None: zeros, the start of an episode).  The observation is
        normalised and masked as ``RecurrentESEngine.act`` does and goes
        through ``ops.lstm_policy_step``; an action is 1 where ``l1 > l0``."""
        x = _core.act_input(self, obs, self.obs_mask)
        if state is None:
            state = tuple(torch.zeros(obs.shape[0], self.cfg.hidden,
                                      device=obs.device) for _ in range(2))
        logits, hnew, cnew = ops.lstm_policy_step(self.theta, x, *state)
        return (logits[:, 1] > logits[:, 0]).to(torch.int64), (hnew, cnew)

    save, load = _core.save, _core.load
