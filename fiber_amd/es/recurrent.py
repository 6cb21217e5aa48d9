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

from .. import ops, tracing
from .engine import ESConfig, make_env_params


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


class RecurrentESEngine:
    def __init__(self, config: ESConfig, ctx=None, device=None,
                 env_params=None, obs_mask=0b1111):
        if ctx is not None:
            raise NotImplementedError(
                "RecurrentESEngine is single-GPU: no ring context")
        self.cfg = config
        if device is None:
            device = torch.device("cuda", 0)
        self.device = device
        if config.pop_per_gpu % 2:
            raise ValueError("pop_per_gpu must be even (antithetic pairs)")
        if not 0 <= int(obs_mask) < 2 ** config.obs_dim:
            raise ValueError("obs_mask must be in [0, %d), got %r"
                             % (2 ** config.obs_dim, obs_mask))
        self.obs_mask = int(obs_mask)
        self.pop_total = config.pop_per_gpu

        self.theta = init_theta_gru(config.seed, device)
        self.adam_m = torch.zeros_like(self.theta)
        self.adam_v = torch.zeros_like(self.theta)
        self.t_step = 0

        if env_params is None:
            self.env_A, self.env_B = make_env_params(config.seed, device)
        else:
            env_A, env_B = env_params
            n = config.obs_dim
            if tuple(env_A.shape) != (n, n) or tuple(env_B.shape) != (n,):
                raise ValueError(
                    "env_params must be (env_A[%d][%d], env_B[%d])"
                    % (n, n, n))
            self.env_A = env_A.detach().to(
                device=device, dtype=torch.float32, copy=True).contiguous()
            self.env_B = env_B.detach().to(
                device=device, dtype=torch.float32, copy=True).contiguous()
        self.obs_sum = torch.zeros(config.obs_dim, device=device)
        self.obs_sumsq = torch.zeros(config.obs_dim, device=device)
        self.obs_count = torch.zeros(1, device=device)
        self.obs_mu = torch.zeros(config.obs_dim, device=device)
        self.obs_nu = torch.ones(config.obs_dim, device=device)

    def _refresh_normaliser(self):
        count = self.obs_count.clamp_min(1.0)
        self.obs_mu = (self.obs_sum / count).contiguous()
        var = self.obs_sumsq / count - self.obs_mu ** 2
        self.obs_nu = var.clamp_min(1e-2).contiguous()

    # -- one ES iteration: ESEngine.step with the rollout swapped ----------
    def step(self, iteration=None):
        cfg = self.cfg
        if iteration is None:
            iteration = self.t_step
        pop = cfg.pop_per_gpu
        with tracing.range("es.rollout_gru"):
            fitness, obs_stat = ops.es_rollout_gru(
                self.theta, cfg.sigma, cfg.seed, iteration, cfg.horizon, 0,
                pop, self.obs_mu, self.obs_nu, self.env_A, self.env_B,
                self.obs_mask)
        ranks = ops.centered_rank(fitness)
        wpair = (ranks[0::2] - ranks[1::2]).contiguous()
        with tracing.range("es.grad"):
            grad = ops.es_grad(wpair, 0, pop // 2, cfg.seed, iteration,
                               self.device, nparams=ops.GRU_NPARAMS)
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

    # -- score the current policy -----------------------------------------
    def evaluate(self, horizon=None, iteration=None):
        """Mean return of the current, unperturbed theta over the 64
        episodes that ``step(iteration)`` starts from: ``es_rollout_gru`` at
        ``sigma = 0`` with two members (one antithetic pair, both the plain
        theta).  Returns a 0-dim device tensor; changes nothing."""
        if horizon is None:
            horizon = self.cfg.horizon
        if iteration is None:
            iteration = self.t_step
        fitness, _ = ops.es_rollout_gru(
            self.theta, 0.0, self.cfg.seed, iteration, horizon, 0, 2,
            self.obs_mu, self.obs_nu, self.env_A, self.env_B, self.obs_mask)
        return fitness[0]

    # -- act with the current policy --------------------------------------
    def act(self, obs, hidden=None):
        """``(actions[n], hidden'[n][64])`` of the current theta for raw
        observations ``obs[n][4]`` and the carried ``hidden`` (None: zeros,
        the start of an episode).  The observation is normalised as
        ``ESEngine.act`` does, its hidden dims set to 0, and goes through
        ``ops.gru_policy_step``; an action is 1 where ``l1 > l0``."""
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
        if hidden is None:
            hidden = torch.zeros(obs.shape[0], self.cfg.hidden,
                                 device=obs.device)
        rstd = torch.rsqrt(self.obs_nu + 1e-4)
        x = ((obs - self.obs_mu) * rstd).clamp_(-5.0, 5.0)
        visible = torch.tensor(
            [(self.obs_mask >> d) & 1 for d in range(self.cfg.obs_dim)],
            dtype=torch.float32, device=obs.device)
        x = (x * visible).contiguous()
        logits, hnew = ops.gru_policy_step(self.theta, x, hidden)
        return (logits[:, 1] > logits[:, 0]).to(torch.int64), hnew

    # -- checkpoint / resume ----------------------------------------------
    def state_dict(self):
        return {
            "theta": self.theta.cpu(),
            "adam_m": self.adam_m.cpu(),
            "adam_v": self.adam_v.cpu(),
            "t_step": self.t_step,
            "obs_sum": self.obs_sum.cpu(),
            "obs_sumsq": self.obs_sumsq.cpu(),
            "obs_count": self.obs_count.cpu(),
            "obs_mask": self.obs_mask,
            "config": dataclasses.asdict(self.cfg),
        }

    def load_state_dict(self, state):
        self.theta.copy_(state["theta"].to(self.device))
        self.adam_m.copy_(state["adam_m"].to(self.device))
        self.adam_v.copy_(state["adam_v"].to(self.device))
        self.t_step = int(state["t_step"])
        self.obs_sum.copy_(state["obs_sum"].to(self.device))
        self.obs_sumsq.copy_(state["obs_sumsq"].to(self.device))
        self.obs_count.copy_(state["obs_count"].to(self.device))
        self.obs_mask = int(state["obs_mask"])
        self._refresh_normaliser()
