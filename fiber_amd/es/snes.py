"""Separable NES on the MLP engine: OpenAI-ES with a step size per
parameter that adapts as the run goes (Wierstra et al., "Natural Evolution
Strategies", the SNES variant; Schaul et al., "High Dimensions and Heavy
Tails for Natural Evolution Strategies").

The state is ``ESEngine``'s plus ``sigma[NPARAMS]``, initialised to
``config.sigma``.  One iteration is:

  1. es_rollout_mlp_sigma — member 2k evaluates theta + sigma * z_k,
                            member 2k+1 evaluates theta - sigma * z_k
                            (sigma, z_k per parameter)
  2. centered_rank        — r = rank transform of the fitness;
                            wdiff[k] = r[2k] - r[2k+1],
                            wsum[k]  = r[2k] + r[2k+1]
  3. es_grad_sigma        — one regeneration of the draws for both rows:
                            g_mu[j]  = sum_k wdiff[k] z_k[j]
                            g_sig[j] = sum_k wsum[k] (z_k[j]^2 - 1)
  4. Adam on theta        — ESEngine.step's lines with grad = g_mu / (pop *
                            config.sigma)
  5. sigma *= exp(0.5 * lr_sigma / pop * g_sig), clamped to
     [sigma_min, sigma_max]; used from the next iteration on
  6. obs-normaliser merge — ESEngine.step's lines

The theta gradient is divided by the scalar *initial* ``config.sigma``, not
by the live vector.  Adam divides each coordinate of its step by the running
root mean square of that coordinate's gradient, so it is invariant to a
fixed rescale per coordinate up to ``adam_eps``: dividing by the live
``sigma[j]`` would buy nothing.  The scalar form makes the engine collapse
to ``ESEngine`` bit for bit when sigma does not move (``lr_sigma = 0``).

The default ``lr_sigma = (3 + ln d) / (5 sqrt(d))`` at d = 4610 is the rule
of the SNES paper, which pairs it with that paper's utility weights; nobody
has tuned it for centered ranks on this workload.  ``sigma_min = 1e-3 *
config.sigma`` and ``sigma_max = 10 * config.sigma`` are guard rails, not
tuned either.

Single process only: the data-parallel version needs a reduce buffer of
2 * NPARAMS gradients and is not built yet.  ``ESPopulation``,
``NoveltyESEngine`` and the conv engine keep a scalar sigma.
"""

import dataclasses
import math

import torch

from .. import ops, tracing
from .engine import ESConfig, ESEngine


def default_lr_sigma(nparams=ops.NPARAMS):
    """(3 + ln d) / (5 sqrt(d)), the SNES paper's rule.  Untuned here."""
    return (3.0 + math.log(nparams)) / (5.0 * math.sqrt(nparams))


@dataclasses.dataclass
class SNESConfig:
    # None: the default described in the module docstring
    lr_sigma: float = None
    sigma_min: float = None
    sigma_max: float = None

    def resolved(self, config: ESConfig):
        """A copy with every None replaced by its default for ``config``."""
        return SNESConfig(
            lr_sigma=(default_lr_sigma() if self.lr_sigma is None
                      else float(self.lr_sigma)),
            sigma_min=(1e-3 * config.sigma if self.sigma_min is None
                       else float(self.sigma_min)),
            sigma_max=(10.0 * config.sigma if self.sigma_max is None
                       else float(self.sigma_max)))


class SNESEngine(ESEngine):
    def __init__(self, config: ESConfig, snes: SNESConfig = None, ctx=None,
                 device=None, env_params=None):
        if ctx is not None:
            raise NotImplementedError(
                "data-parallel separable NES is not built yet: both gradient "
                "rows (2 * NPARAMS floats) would have to be all-reduced; run "
                "SNESEngine in one process (ctx=None)")
        if snes is None:
            snes = SNESConfig()
        snes = snes.resolved(config)
        if not snes.lr_sigma >= 0.0 or math.isinf(snes.lr_sigma):
            raise ValueError("lr_sigma must be finite and >= 0, got %r"
                             % snes.lr_sigma)
        if not 0.0 <= snes.sigma_min <= snes.sigma_max < math.inf:
            raise ValueError("need 0 <= sigma_min <= sigma_max < inf, got "
                             "%r, %r" % (snes.sigma_min, snes.sigma_max))
        if not 0.0 <= config.sigma < math.inf:
            raise ValueError("sigma must be finite and >= 0, got %r"
                             % config.sigma)
        super().__init__(config, ctx=None, device=device,
                         env_params=env_params)
        self.snes = snes
        self.sigma = torch.full((ops.NPARAMS,), float(config.sigma),
                                dtype=torch.float32, device=self.device)

    # -- one SNES iteration ------------------------------------------------
    def step(self, iteration=None):
        cfg, snes = self.cfg, self.snes
        if iteration is None:
            iteration = self.t_step
        shard = cfg.pop_per_gpu

        with tracing.range("snes.rollout"):
            fitness, obs_stat = ops.es_rollout_mlp_sigma(
                self.theta, self.sigma, cfg.seed, iteration, cfg.horizon, 0,
                shard, self.obs_mu, self.obs_nu, self.env_A, self.env_B)

        ranks = ops.centered_rank(fitness)
        wdiff = (ranks[0::2] - ranks[1::2]).contiguous()
        wsum = (ranks[0::2] + ranks[1::2]).contiguous()

        with tracing.range("snes.grad"):
            grad, g_sig = ops.es_grad_sigma(wdiff, wsum, 0, shard // 2,
                                            cfg.seed, iteration, self.device)
        # the scalar initial sigma: see the module docstring
        grad /= float(self.pop_total) * cfg.sigma

        # maximize fitness => ascend (ESEngine.step's Adam)
        self.t_step += 1
        b1, b2 = cfg.adam_beta1, cfg.adam_beta2
        self.adam_m.mul_(b1).add_(grad, alpha=1 - b1)
        self.adam_v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
        mhat = self.adam_m / (1 - b1 ** self.t_step)
        vhat = self.adam_v / (1 - b2 ** self.t_step)
        self.theta.add_(cfg.lr * mhat / (vhat.sqrt() + cfg.adam_eps))

        # step sizes (applied next iteration)
        self.sigma.mul_(
            torch.exp(g_sig * (0.5 * snes.lr_sigma / self.pop_total))
        ).clamp_(snes.sigma_min, snes.sigma_max)

        # running obs normalization (applied next iteration)
        self.obs_sum += obs_stat[: cfg.obs_dim]
        self.obs_sumsq += obs_stat[cfg.obs_dim : 2 * cfg.obs_dim]
        self.obs_count += obs_stat[2 * cfg.obs_dim]
        count = self.obs_count.clamp_min(1.0)
        self.obs_mu = (self.obs_sum / count).contiguous()
        var = self.obs_sumsq / count - self.obs_mu ** 2
        self.obs_nu = var.clamp_min(1e-2).contiguous()

        return {
            "fitness_mean": float(fitness.mean()),
            "fitness_max": float(fitness.max()),
            "grad_norm": float(grad.norm()),
            "rollouts": self.pop_total * cfg.envs_per_member,
            "env_steps": self.pop_total * cfg.envs_per_member * cfg.horizon,
            "sigma_mean": float(self.sigma.mean()),
            "sigma_min": float(self.sigma.min()),
            "sigma_max": float(self.sigma.max()),
        }

    # -- checkpoint / resume ----------------------------------------------
    def state_dict(self):
        state = super().state_dict()
        state["sigma"] = self.sigma.cpu()
        state["snes_config"] = dataclasses.asdict(self.snes)
        return state

    def load_state_dict(self, state):
        if "sigma" not in state:
            raise ValueError("the checkpoint holds no sigma vector: it is "
                             "not an SNESEngine's")
        if tuple(state["sigma"].shape) != tuple(self.sigma.shape):
            raise ValueError("checkpoint sigma has shape %s, engine %s"
                             % (tuple(state["sigma"].shape),
                                tuple(self.sigma.shape)))
        super().load_state_dict(state)
        self.sigma.copy_(state["sigma"].to(self.device))
        self.snes = SNESConfig(**state["snes_config"])
