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

from .. import ops, tracing
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
    ``state_dict`` / ``load_state_dict``, ``save`` / ``load``) on the LSTM
    kernels; ``act`` carries the pair ``(h, c)``."""

    def __init__(self, config, ctx=None, device=None, env_params=None,
                 obs_mask=0b1111):
        if ctx is not None:
            raise NotImplementedError(
                "LSTMESEngine is single-GPU: no ring context")
        super().__init__(config, None, device, env_params, obs_mask)
        self.theta = init_theta_lstm(config.seed, self.device)
        self.adam_m = torch.zeros_like(self.theta)
        self.adam_v = torch.zeros_like(self.theta)

    def _rollout(self, sigma, iteration, horizon, pop):
        return ops.es_rollout_lstm(
            self.theta, sigma, self.cfg.seed, iteration, horizon, 0, pop,
            self.obs_mu, self.obs_nu, self.env_A, self.env_B, self.obs_mask)

    # -- one ES iteration: RecurrentESEngine.step with the rollout swapped --
    def step(self, iteration=None):
        cfg = self.cfg
        if iteration is None:
            iteration = self.t_step
        pop = cfg.pop_per_gpu
        with tracing.range("es.rollout_lstm"):
            fitness, obs_stat = self._rollout(cfg.sigma, iteration,
                                              cfg.horizon, pop)
        ranks = ops.centered_rank(fitness)
        wpair = (ranks[0::2] - ranks[1::2]).contiguous()
        with tracing.range("es.grad"):
            grad = ops.es_grad(wpair, 0, pop // 2, cfg.seed, iteration,
                               self.device, nparams=ops.LSTM_NPARAMS)
        grad /= float(pop) * cfg.sigma

        self.t_step += 1
        b1, b2 = cfg.adam_beta1, cfg.adam_beta2
        self.adam_m.mul_(b1).add_(grad, alpha=1 - b1)
        self.adam_v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
        mhat = self.adam_m / (1 - b1 ** self.t_step)
        vhat = self.adam_v / (1 - b2 ** self.t_step)
        self.theta.add_(cfg.lr * mhat / (vhat.sqrt() + cfg.adam_eps))

        self.obs_sum += obs_stat[: cfg.obs_dim]
        self.obs_sumsq += obs_stat[cfg.obs_dim : 2 * cfg.obs_dim]
        self.obs_count += obs_stat[2 * cfg.obs_dim]
        self._refresh_normaliser()
        return {
            "fitness_mean": float(fitness.mean()),
            "fitness_max": float(fitness.max()),
            "grad_norm": float(grad.norm()),
            "rollouts": pop * cfg.envs_per_member,
            "env_steps": pop * cfg.envs_per_member * cfg.horizon,
        }

    def evaluate(self, horizon=None, iteration=None):
        """Mean return of the current, unperturbed theta over the 64
        episodes that ``step(iteration)`` starts from: ``es_rollout_lstm`` at
        ``sigma = 0`` with two members.  Returns a 0-dim device tensor;
        changes nothing."""
        if horizon is None:
            horizon = self.cfg.horizon
        if iteration is None:
            iteration = self.t_step
        return self._rollout(0.0, iteration, horizon, 2)[0][0]

    def act(self, obs, state=None):
        """``(actions[n], (h'[n][64], c'[n][64]))`` of the current theta for
        raw observations ``obs[n][4]`` and the carried ``state = (h, c)``
        (None: zeros, the start of an episode).  The observation is
        normalised and masked as ``RecurrentESEngine.act`` does and goes
        through ``ops.lstm_policy_step``; an action is 1 where ``l1 > l0``."""
        if not torch.is_tensor(obs):
            raise TypeError("obs must be a tensor, got %s"
                            % type(obs).__name__)
        if obs.dim() != 2 or obs.shape[1] != self.cfg.obs_dim:
            raise ValueError("obs must be [n, %d], got %s"
                             % (self.cfg.obs_dim, tuple(obs.shape)))
        if obs.dtype != torch.float32:
            raise TypeError("obs must be torch.float32, got %s" % obs.dtype)
        if obs.device != self.theta.device:
            raise TypeError("obs is on %s, the engine on %s"
                            % (obs.device, self.theta.device))
        if state is None:
            state = tuple(torch.zeros(obs.shape[0], self.cfg.hidden,
                                      device=obs.device) for _ in range(2))
        rstd = torch.rsqrt(self.obs_nu + 1e-4)
        x = ((obs - self.obs_mu) * rstd).clamp_(-5.0, 5.0)
        visible = torch.tensor(
            [(self.obs_mask >> d) & 1 for d in range(self.cfg.obs_dim)],
            dtype=torch.float32, device=obs.device)
        x = (x * visible).contiguous()
        logits, hnew, cnew = ops.lstm_policy_step(self.theta, x, *state)
        return (logits[:, 1] > logits[:, 0]).to(torch.int64), (hnew, cnew)

    def save(self, path):
        torch.save(self.state_dict(), path)

    def load(self, path):
        self.load_state_dict(torch.load(path, weights_only=False))
