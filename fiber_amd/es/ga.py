"""Deep GA on the MLP engine: the gradient-free line of deep neuroevolution
(Such et al., "Deep Neuroevolution: Genetic Algorithms Are a Competitive
Alternative for Training Deep Neural Networks for Reinforcement Learning").

A population of mutated copies is evaluated, the best ``truncation`` survive,
and the next generation is the best ``n_elite`` survivors as they are plus
Gaussian mutations of uniformly drawn survivors.  An individual is stored as
its chain of mutation seeds, not as its weights: every mutation is
regenerated from Philox counters (seed, generation, child slot), the draw
``es_rollout_mlp`` uses for pair ``slot`` at iteration ``generation``.

The state is ``theta0 = init_theta(seed)``, the materialised survivors
``parents[T_cur][NPARAMS]`` (one row, ``theta0``, before the first step;
``truncation`` rows afterwards, best first), their seed chains
``lineage[T_cur][cap]`` (int32 on the device: column c holds the slot applied
in generation c, or -1 for a generation the genome passed through as an
unmutated elite; the capacity doubles when full), ``generation`` and
``ESEngine``'s obs normaliser.  One generation is:

  1. ga_parents      — parent_idx[pop], slot[pop]: members below n_elite are
                       the survivors of that rank, unmutated; every other
                       member m mutates a drawn survivor with the draw of
                       slot m
  2. ga_rollout_mlp  — ONE launch: every member's own parent row and draw
                       go straight into LDS, nothing is materialised
  3. ga_truncate     — order[truncation], exact and reproducible tie order
  4. ga_survivors    — the weights the survivors were evaluated with, out of
                       place; the lineage gather beside it is torch indexing
  5. obs-normaliser merge — ESEngine.step's lines

``parents`` is a cache of ``ga_decode(theta0, lineage)``, which rebuilds it
bit for bit; a checkpoint therefore stores the chains (truncation x
generation x 4 bytes) and not the weights (truncation x 18 KB).

Out of scope: the paper's separate 30-episode re-evaluation of the elite
candidates (every member here already averages 64 episodes; the elites are
re-scored with everyone else on each generation's start states), crossover,
an adaptive or per-parameter sigma, the conv engine, ``ESPopulation`` and
multi-process runs.  A per-parent, per-parameter step from output gradients
(safe mutations) is ``SafeGAEngine`` in fiber_amd/es/safe_ga.py.
"""

import dataclasses
import math

import numpy as np
import torch

from .. import ops, tracing
from .engine import init_theta, make_env_params


@dataclasses.dataclass
class GAConfig:
    pop: int = 1024
    truncation: int = 32          # survivors per generation
    n_elite: int = 1              # survivors copied unmutated
    sigma: float = 0.02           # mutation step, constant
    horizon: int = 200
    seed: int = 1234
    # fixed by the compiled kernel:
    obs_dim: int = ops.OBS_DIM
    envs_per_member: int = ops.ENVS_PER_MEMBER

    def __post_init__(self):
        self.validate()

    def validate(self):
        """ValueError unless 1 <= n_elite <= truncation <= pop, 2 <= pop <=
        65536 (what ga_truncate ranks), truncation <= 65535, horizon >= 1
        and sigma finite and >= 0."""
        if not 1 <= self.n_elite <= self.truncation <= self.pop:
            raise ValueError(
                "need 1 <= n_elite <= truncation <= pop, got n_elite %r, "
                "truncation %r, pop %r"
                % (self.n_elite, self.truncation, self.pop))
        if not 2 <= self.pop <= ops.GA_TRUNCATE_MAX:
            raise ValueError("pop must be in [2, %d], got %r"
                             % (ops.GA_TRUNCATE_MAX, self.pop))
        if self.truncation > ops.GA_ROWS_MAX:
            raise ValueError("truncation must be <= %d, got %r"
                             % (ops.GA_ROWS_MAX, self.truncation))
        if self.horizon < 1:
            raise ValueError("horizon must be >= 1, got %r" % self.horizon)
        if not 0.0 <= self.sigma < math.inf:  # also refuses a NaN
            raise ValueError("sigma must be finite and >= 0, got %r"
                             % self.sigma)


class GAEngine:
    def __init__(self, config: GAConfig, ctx=None, device=None,
                 env_params=None):
        if ctx is not None:
            raise NotImplementedError(
                "data-parallel Deep GA is not built yet: the fitness would "
                "have to be all-gathered before the truncation; run GAEngine "
                "in one process (ctx=None)")
        config.validate()
        self.cfg = config
        if device is None:
            device = torch.device("cuda", 0)
        self.device = device

        self.theta0 = init_theta(config.seed, device)
        self.parents = self.theta0.unsqueeze(0).clone()
        self.lineage = torch.full((1, 8), -1, dtype=torch.int32,
                                  device=device)
        self.generation = 0

        # env_params = (env_A[4][4], env_B[4]) as for ESEngine; not part of
        # state_dict().
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

        # what the last step launched and chose, for inspection and tests
        self.last = None

    @property
    def theta(self):
        """The best survivor of the last generation (theta0 before the
        first)."""
        return self.parents[0]

    # -- one generation ------------------------------------------------------
    def step(self):
        cfg = self.cfg
        g = self.generation
        T_cur = self.parents.shape[0]
        # generation 0 has the one parent theta0: at most one elite
        n_elite = min(cfg.n_elite, T_cur)

        parent_idx, slot = ops.ga_parents(cfg.seed, g, cfg.pop, n_elite,
                                          T_cur, self.device)
        with tracing.range("ga.rollout"):
            fitness, obs_stat = ops.ga_rollout_mlp(
                self.parents, parent_idx, slot, cfg.sigma, cfg.seed, g,
                cfg.horizon, self.obs_mu, self.obs_nu, self.env_A,
                self.env_B)
        order = ops.ga_truncate(fitness, cfg.truncation)
        with tracing.range("ga.survivors"):
            new_parents = ops.ga_survivors(self.parents, parent_idx, slot,
                                           order, cfg.sigma, cfg.seed, g)

        # seed chains of the survivors (plumbing: torch indexing)
        cap = self.lineage.shape[1]
        if g >= cap:
            cap *= 2
        chosen = order.long()
        lineage = torch.full((cfg.truncation, cap), -1, dtype=torch.int32,
                             device=self.device)
        lineage[:, :g] = self.lineage[parent_idx[chosen].long(), :g]
        lineage[:, g] = slot[chosen]

        self.parents, self.lineage = new_parents, lineage
        self.generation = g + 1
        self.last = {"fitness": fitness, "parent_idx": parent_idx,
                     "slot": slot, "order": order}

        # running obs normalization (applied next generation)
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
            # member 0: the best survivor of the generation before, scored
            # again, unmutated, on this generation's episodes
            "elite_fitness": float(fitness[0]),
            "rollouts": cfg.pop * cfg.envs_per_member,
            "env_steps": cfg.pop * cfg.envs_per_member * cfg.horizon,
            "generation": self.generation,   # generations completed
        }

    # -- score the best survivor ---------------------------------------------
    def evaluate(self, horizon=None, iteration=None, return_episodes=False):
        """Mean return of ``theta``, unmutated, on this engine's environment
        with its current obs normaliser: one es_eval_matrix launch with K =
        M = 1, as ESEngine.evaluate.  The 64 episodes start from the states
        generation ``iteration`` uses (default: the next one).  Changes
        nothing in the engine."""
        if horizon is None:
            horizon = self.cfg.horizon
        if iteration is None:
            iteration = self.generation
        out = ops.es_eval_matrix(
            self.theta.unsqueeze(0), self.obs_mu.unsqueeze(0),
            self.obs_nu.unsqueeze(0), self.env_A.unsqueeze(0),
            self.env_B.unsqueeze(0), self.cfg.seed, iteration, horizon,
            return_episodes=return_episodes)
        if return_episodes:
            scores, episodes = out
            return scores.reshape(()), episodes.reshape(-1)
        return out.reshape(())

    # -- the compact encoding --------------------------------------------------
    def genome(self, t):
        """The seed chain of survivor ``t``: an int32 CPU tensor
        [generation], entry c the child slot whose draw was applied in
        generation c, or -1."""
        if not 0 <= t < self.lineage.shape[0]:
            raise IndexError("survivor %r of %d" % (t, self.lineage.shape[0]))
        return self.lineage[t, : self.generation].cpu()

    def decode(self, lineage_rows):
        """Weights [N][NPARAMS] of the seed chains ``lineage_rows`` (int,
        [N][G] or one chain [G]; a tensor, an array or nested lists), rebuilt
        from ``theta0`` with this engine's sigma and seed by ga_decode."""
        if not torch.is_tensor(lineage_rows):
            lineage_rows = torch.from_numpy(
                np.asarray(lineage_rows, dtype=np.int32))
        if lineage_rows.dim() == 1:
            lineage_rows = lineage_rows.unsqueeze(0)
        rows = lineage_rows.to(device=self.device,
                               dtype=torch.int32).contiguous()
        return ops.ga_decode(self.theta0, rows, self.cfg.sigma,
                             self.cfg.seed)

    # -- checkpoint / resume -------------------------------------------------
    def state_dict(self):
        """theta0, the seed chains, the obs sums and the config; not the
        weights, which load_state_dict() decodes again."""
        return {
            "theta0": self.theta0.cpu(),
            "lineage": self.lineage[:, : self.generation].cpu(),
            "generation": self.generation,
            "obs_sum": self.obs_sum.cpu(),
            "obs_sumsq": self.obs_sumsq.cpu(),
            "obs_count": self.obs_count.cpu(),
            "config": dataclasses.asdict(self.cfg),
        }

    def load_state_dict(self, state):
        """Rebuild ``parents`` from the saved chains with ga_decode.  The
        checkpoint's sigma and seed must be this engine's (ValueError
        otherwise): the chains mean nothing under other draws.  pop,
        truncation, n_elite and horizon are not compared, and the saved
        number of chains need not be ``truncation``: the next step() then
        breeds from the ``T_cur`` saved survivors, with at most ``T_cur``
        elites, and leaves ``truncation`` rows as usual."""
        if "lineage" not in state or "theta0" not in state:
            raise ValueError("the checkpoint holds no seed chains: it is "
                             "not a GAEngine's")
        saved = state["config"]
        # the chains mean these weights only with the sigma and seed that
        # drew them
        for key in ("sigma", "seed"):
            if saved[key] != getattr(self.cfg, key):
                raise ValueError("the checkpoint was written with %s = %r, "
                                 "this engine has %r"
                                 % (key, saved[key], getattr(self.cfg, key)))
        generation = int(state["generation"])
        lineage = state["lineage"]
        if lineage.dim() != 2 or lineage.shape[1] != generation \
                or lineage.shape[0] < 1:
            raise ValueError("checkpoint lineage has shape %s at generation "
                             "%d" % (tuple(lineage.shape), generation))
        if tuple(state["theta0"].shape) != tuple(self.theta0.shape):
            raise ValueError("checkpoint theta0 has shape %s"
                             % (tuple(state["theta0"].shape),))
        self.theta0.copy_(state["theta0"].to(self.device))
        rows = lineage.to(device=self.device, dtype=torch.int32).contiguous()
        self.parents = ops.ga_decode(self.theta0, rows, self.cfg.sigma,
                                     self.cfg.seed)
        cap = 8
        while cap < generation:
            cap *= 2
        self.lineage = torch.full((rows.shape[0], cap), -1,
                                  dtype=torch.int32, device=self.device)
        self.lineage[:, :generation] = rows
        self.generation = generation
        self.last = None
        self.obs_sum.copy_(state["obs_sum"].to(self.device))
        self.obs_sumsq.copy_(state["obs_sumsq"].to(self.device))
        self.obs_count.copy_(state["obs_count"].to(self.device))
        count = self.obs_count.clamp_min(1.0)
        self.obs_mu = (self.obs_sum / count).contiguous()
        var = self.obs_sumsq / count - self.obs_mu ** 2
        self.obs_nu = var.clamp_min(1e-2).contiguous()

    def save(self, path):
        torch.save(self.state_dict(), path)

    def load(self, path):
        self.load_state_dict(torch.load(path, weights_only=False))
