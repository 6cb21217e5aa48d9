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

from .. import ops, tracing
from .engine import ESConfig, make_env_params


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


class WideESEngine:
    def __init__(self, config: ESConfig, hidden, ctx=None, device=None,
                 env_params=None):
        if ctx is not None:
            raise NotImplementedError(
                "WideESEngine is single-GPU: no ring context")
        self.nparams = ops.wide_nparams(hidden)   # refuses 64 and the rest
        self.hidden = int(hidden)
        self.cfg = config
        if device is None:
            device = torch.device("cuda", 0)
        self.device = device
        if config.pop_per_gpu % 2:
            raise ValueError("pop_per_gpu must be even (antithetic pairs)")
        self.pop_total = config.pop_per_gpu

        self.theta = init_theta_wide(config.seed, self.hidden, device)
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
        with tracing.range("es.rollout_wide"):
            fitness, obs_stat = ops.es_rollout_mlp_wide(
                self.theta, self.hidden, cfg.sigma, cfg.seed, iteration,
                cfg.horizon, 0, pop, self.obs_mu, self.obs_nu, self.env_A,
                self.env_B)
        ranks = ops.centered_rank(fitness)
        wpair = (ranks[0::2] - ranks[1::2]).contiguous()
        with tracing.range("es.grad"):
            grad = ops.es_grad(wpair, 0, pop // 2, cfg.seed, iteration,
                               self.device, nparams=self.nparams)
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
        episodes that ``step(iteration)`` starts from:
        ``es_rollout_mlp_wide`` at ``sigma = 0`` with two members (one
        antithetic pair, both the plain theta).  Returns a 0-dim device
        tensor; changes nothing."""
        if horizon is None:
            horizon = self.cfg.horizon
        if iteration is None:
            iteration = self.t_step
        fitness, _ = ops.es_rollout_mlp_wide(
            self.theta, self.hidden, 0.0, self.cfg.seed, iteration, horizon,
            0, 2, self.obs_mu, self.obs_nu, self.env_A, self.env_B)
        return fitness[0]

    # -- act with the current policy --------------------------------------
    def act(self, obs, return_logits=False):
        """Actions of the current theta for raw observations ``obs[n][4]``
        (fp32, on this engine's device): normalised as ``ESEngine.act``
        does and sent through ``ops.mlp_policy_forward_wide``.  Returns
        int64 ``actions[n]``, 1 where ``l1 > l0`` (a tie is 0), or
        ``(actions, logits)``.  The serving kernel keeps ``h2`` in fp32 as
        the step loop does, so both choose alike."""
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
        rstd = torch.rsqrt(self.obs_nu + 1e-4)
        x = ((obs - self.obs_mu) * rstd).clamp_(-5.0, 5.0).contiguous()
        logits = ops.mlp_policy_forward_wide(self.theta, self.hidden, x)
        actions = (logits[:, 1] > logits[:, 0]).to(torch.int64)
        if return_logits:
            return actions, logits
        return actions

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
            "hidden": self.hidden,
            "config": dataclasses.asdict(self.cfg),
        }

    def load_state_dict(self, state):
        if int(state["hidden"]) != self.hidden:
            raise ValueError("checkpoint has hidden = %d, the engine %d"
                             % (int(state["hidden"]), self.hidden))
        self.theta.copy_(state["theta"].to(self.device))
        self.adam_m.copy_(state["adam_m"].to(self.device))
        self.adam_v.copy_(state["adam_v"].to(self.device))
        self.t_step = int(state["t_step"])
        self.obs_sum.copy_(state["obs_sum"].to(self.device))
        self.obs_sumsq.copy_(state["obs_sumsq"].to(self.device))
        self.obs_count.copy_(state["obs_count"].to(self.device))
        self._refresh_normaliser()

    def save(self, path):
        torch.save(self.state_dict(), path)

    def load(self, path):
        self.load_state_dict(torch.load(path, weights_only=False))
