"""Novelty-seeking ES on the MLP engine: NS-ES, NSR-ES and NSRA-ES
(Conti et al., "Improving Exploration in Evolution Strategies for Deep
Reinforcement Learning via a Population of Novelty-Seeking Agents").

A member's behaviour characterisation (BC) is the mean over its 64
episodes of the final state s_H, 4 floats, reported by the rollout kernel
itself (``ops.es_rollout_mlp_bc``).  Its novelty is the mean Euclidean
distance to the k nearest BCs of an archive (``ops.bc_knn_novelty``,
k <= 16).  One iteration of the engine is:

  1. pick an agent of the meta-population, in proportion to the novelty
     of its current BC
  2. es_rollout_mlp_bc   — fitness, obs statistics and BC of every member
  3. bc_knn_novelty      — novelty of every member against the archive
  4. centered_rank of fitness and of novelty, combined per mode:
       ns    novelty ranks alone
       nsr   the average of the two
       nsra  w * fitness + (1 - w) * novelty, w adapted as the run goes
  5. es_grad + Adam on the chosen agent, the arithmetic of ESEngine.step
  6. es_eval_bc on the updated agent: its BC joins the archive, its score
     drives the nsra schedule

With equal member weights the update is bit-identical to ESEngine's
(``mode="nsra", weight=1.0, weight_delta=0.0``).  BCs must be finite; a
diverged policy whose states overflow gives an unspecified novelty.

Single process only: gathering BCs across ranks is not built yet.
"""

import dataclasses

import torch

from .. import ops, tracing
from .engine import ESConfig, init_theta, make_env_params

MODES = ("ns", "nsr", "nsra")


@dataclasses.dataclass
class NoveltyConfig:
    mode: str = "nsr"             # "ns", "nsr" or "nsra"
    k: int = 10                   # neighbours per novelty, <= ops.BC_KNN_MAX
    meta_size: int = 1            # agents in the meta-population
    archive_capacity: int = 4096  # BCs kept, first in first out
    weight: float = 1.0           # nsra only: initial fitness weight w
    weight_delta: float = 0.05    # nsra only: step of w
    patience: int = 10            # nsra only: stalled steps before w drops


class NoveltyESEngine:
    def __init__(self, config: ESConfig, novelty: NoveltyConfig = None,
                 ctx=None, device=None, env_params=None):
        if ctx is not None:
            raise NotImplementedError(
                "data-parallel novelty search is not built yet: the BCs of "
                "all ranks would have to be gathered before the novelty "
                "ranks; run NoveltyESEngine in one process (ctx=None)")
        if novelty is None:
            novelty = NoveltyConfig()
        self.cfg = config
        self.ncfg = novelty
        if device is None:
            device = torch.device("cuda", 0)
        self.device = device
        if config.pop_per_gpu % 2 or config.pop_per_gpu < 2:
            raise ValueError("pop_per_gpu must be even and >= 2 "
                             "(antithetic pairs)")
        if novelty.mode not in MODES:
            raise ValueError("mode must be one of %s, got %r"
                             % (MODES, novelty.mode))
        if not 1 <= novelty.k <= ops.BC_KNN_MAX:
            raise ValueError("k must be in [1, %d], got %d"
                             % (ops.BC_KNN_MAX, novelty.k))
        if novelty.meta_size < 1:
            raise ValueError("meta_size must be >= 1")
        if novelty.archive_capacity < novelty.meta_size:
            raise ValueError("archive_capacity must hold the BC of every "
                             "agent")
        if not 0.0 <= novelty.weight <= 1.0:
            raise ValueError("weight must be in [0, 1]")
        if novelty.patience < 1:
            raise ValueError("patience must be >= 1")
        self.pop_total = config.pop_per_gpu
        n_agents = novelty.meta_size

        # agent m is row m of each tensor
        self.thetas = torch.stack(
            [init_theta(config.seed + m, device) for m in range(n_agents)]
        ).contiguous()
        self.adam_m = torch.zeros_like(self.thetas)
        self.adam_v = torch.zeros_like(self.thetas)
        self.t_steps = [0] * n_agents
        # noise / env-init counter of the next step, over all agents
        self.iteration = 0

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
        # one obs normaliser shared by all agents
        self.obs_sum = torch.zeros(config.obs_dim, device=device)
        self.obs_sumsq = torch.zeros(config.obs_dim, device=device)
        self.obs_count = torch.zeros(1, device=device)
        self.obs_mu = torch.zeros(config.obs_dim, device=device)
        self.obs_nu = torch.ones(config.obs_dim, device=device)

        # archive: a ring of archive_capacity rows; row total % capacity is
        # the next one written, the first min(total, capacity) are valid
        self.archive = torch.zeros(novelty.archive_capacity, ops.BC_DIM,
                                   device=device)
        self.archive_total = 0
        self.agent_bc = torch.zeros(n_agents, ops.BC_DIM, device=device)

        # nsra state
        self.weight = float(novelty.weight)
        self.best_score = float("-inf")
        self.stall = 0

        self._gen = torch.Generator().manual_seed(config.seed)

        self.last_agent = None
        self.last_fitness = None
        self.last_bc = None
        self.last_novelty = None
        self.last_weights = None

        # the BC of every agent, from one launch
        rep = lambda t: t.unsqueeze(0).expand(  # noqa: E731
            n_agents, *t.shape).contiguous()
        _scores, bc = ops.es_eval_bc(
            self.thetas, rep(self.obs_mu), rep(self.obs_nu),
            self.env_A.unsqueeze(0), self.env_B.unsqueeze(0), config.seed,
            self.iteration, config.horizon)
        self.agent_bc.copy_(bc[:, 0])
        for m in range(n_agents):
            self._archive_append(self.agent_bc[m])

    # -- archive -------------------------------------------------------------
    @property
    def archive_size(self):
        return min(self.archive_total, self.ncfg.archive_capacity)

    def _archive_append(self, bc):
        self.archive[self.archive_total % self.ncfg.archive_capacity].copy_(
            bc)
        self.archive_total += 1

    def archive_rows(self):
        """The archived BCs, oldest first (a copy)."""
        cap = self.ncfg.archive_capacity
        if self.archive_total <= cap:
            return self.archive[: self.archive_total].clone()
        head = self.archive_total % cap
        return torch.cat([self.archive[head:], self.archive[:head]])

    def _novelty(self, bc):
        size = self.archive_size
        return ops.bc_knn_novelty(bc, self.archive[:size],
                                  min(self.ncfg.k, size))

    # -- agent choice -----------------------------------------------------------
    def choice_probabilities(self):
        """float64 CPU tensor [meta_size]: in proportion to the novelty of
        each agent's current BC against the archive, uniform if all are
        0."""
        nov = self._novelty(self.agent_bc).cpu().double()
        total = nov.sum()
        if float(total) == 0.0:
            return torch.full_like(nov, 1.0 / nov.numel())
        return nov / total

    def _choose_agent(self):
        if self.ncfg.meta_size == 1:
            return 0
        probs = self.choice_probabilities()
        return int(torch.multinomial(probs, 1, generator=self._gen))

    # -- one iteration -----------------------------------------------------------
    def step(self, iteration=None):
        cfg, ncfg = self.cfg, self.ncfg
        if iteration is None:
            iteration = self.iteration
        shard = cfg.pop_per_gpu
        agent = self._choose_agent()
        theta = self.thetas[agent]
        adam_m = self.adam_m[agent]
        adam_v = self.adam_v[agent]

        with tracing.range("ns.rollout"):
            fitness, obs_stat, bc = ops.es_rollout_mlp_bc(
                theta, cfg.sigma, cfg.seed, iteration, cfg.horizon, 0,
                shard, self.obs_mu, self.obs_nu, self.env_A, self.env_B)
        with tracing.range("ns.novelty"):
            novelty = self._novelty(bc)

        rf = ops.centered_rank(fitness)
        rn = ops.centered_rank(novelty)
        if ncfg.mode == "ns":
            weights = rn
        elif ncfg.mode == "nsr":
            weights = 0.5 * (rf + rn)
        else:
            weights = self.weight * rf + (1.0 - self.weight) * rn
        wpair = (weights[0::2] - weights[1::2]).contiguous()

        with tracing.range("es.grad"):
            grad = ops.es_grad(wpair, 0, shard // 2, cfg.seed, iteration,
                               self.device)
        grad /= float(self.pop_total) * cfg.sigma

        # ascend: ESEngine.step's Adam, on the chosen agent's rows
        self.t_steps[agent] += 1
        t_step = self.t_steps[agent]
        b1, b2 = cfg.adam_beta1, cfg.adam_beta2
        adam_m.mul_(b1).add_(grad, alpha=1 - b1)
        adam_v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
        mhat = adam_m / (1 - b1 ** t_step)
        vhat = adam_v / (1 - b2 ** t_step)
        theta.add_(cfg.lr * mhat / (vhat.sqrt() + cfg.adam_eps))

        # running obs normalization (applied next iteration)
        self.obs_sum += obs_stat[: cfg.obs_dim]
        self.obs_sumsq += obs_stat[cfg.obs_dim : 2 * cfg.obs_dim]
        self.obs_count += obs_stat[2 * cfg.obs_dim]
        count = self.obs_count.clamp_min(1.0)
        self.obs_mu = (self.obs_sum / count).contiguous()
        var = self.obs_sumsq / count - self.obs_mu ** 2
        self.obs_nu = var.clamp_min(1e-2).contiguous()

        self.iteration = iteration + 1

        # the updated agent, with the updated normaliser, from the states
        # the next step starts from: its BC joins the archive
        with tracing.range("ns.eval"):
            scores, agent_bc = ops.es_eval_bc(
                theta.unsqueeze(0), self.obs_mu.unsqueeze(0),
                self.obs_nu.unsqueeze(0), self.env_A.unsqueeze(0),
                self.env_B.unsqueeze(0), cfg.seed, self.iteration,
                cfg.horizon)
        self.agent_bc[agent].copy_(agent_bc[0, 0])
        self._archive_append(agent_bc[0, 0])
        score = float(scores[0, 0])

        used_weight = self.weight
        if ncfg.mode == "nsra":
            if score > self.best_score:
                self.best_score = score
                self.weight = min(1.0, self.weight + ncfg.weight_delta)
                self.stall = 0
            else:
                self.stall += 1
                if self.stall >= ncfg.patience:
                    self.weight = max(0.0, self.weight - ncfg.weight_delta)
                    self.stall = 0

        self.last_agent = agent
        self.last_fitness = fitness
        self.last_bc = bc
        self.last_novelty = novelty
        self.last_weights = weights

        return {
            "fitness_mean": float(fitness.mean()),
            "fitness_max": float(fitness.max()),
            "grad_norm": float(grad.norm()),
            "rollouts": self.pop_total * cfg.envs_per_member,
            "env_steps": self.pop_total * cfg.envs_per_member * cfg.horizon,
            "novelty_mean": float(novelty.mean()),
            # the fitness weight this step's update used (nsra; the fixed
            # 0 and 0.5 of ns and nsr otherwise)
            "weight": {"ns": 0.0, "nsr": 0.5}.get(ncfg.mode, used_weight),
            "agent": agent,
            "agent_score": score,
            "archive_size": self.archive_size,
        }

    # -- score an agent ---------------------------------------------------------
    def evaluate(self, agent=0, horizon=None, iteration=None,
                 return_episodes=False):
        """Mean return of agent ``agent``'s current, unperturbed theta with
        the current obs normaliser: ESEngine.evaluate for the agent named.
        Changes nothing in the engine."""
        if not 0 <= agent < self.ncfg.meta_size:
            raise ValueError("agent must be in [0, %d), got %d"
                             % (self.ncfg.meta_size, agent))
        if horizon is None:
            horizon = self.cfg.horizon
        if iteration is None:
            iteration = self.iteration
        out = ops.es_eval_matrix(
            self.thetas[agent].unsqueeze(0), self.obs_mu.unsqueeze(0),
            self.obs_nu.unsqueeze(0), self.env_A.unsqueeze(0),
            self.env_B.unsqueeze(0), self.cfg.seed, iteration, horizon,
            return_episodes=return_episodes)
        if return_episodes:
            scores, episodes = out
            return scores.reshape(()), episodes.reshape(-1)
        return out.reshape(())

    # -- checkpoint / resume ------------------------------------------------------
    def state_dict(self):
        return {
            "thetas": self.thetas.cpu(),
            "adam_m": self.adam_m.cpu(),
            "adam_v": self.adam_v.cpu(),
            "t_steps": list(self.t_steps),
            "iteration": self.iteration,
            "obs_sum": self.obs_sum.cpu(),
            "obs_sumsq": self.obs_sumsq.cpu(),
            "obs_count": self.obs_count.cpu(),
            "archive": self.archive.cpu(),
            "archive_total": self.archive_total,
            "agent_bc": self.agent_bc.cpu(),
            "weight": self.weight,
            "best_score": self.best_score,
            "stall": self.stall,
            "generator": self._gen.get_state(),
            "config": dataclasses.asdict(self.cfg),
            "novelty_config": dataclasses.asdict(self.ncfg),
        }

    def load_state_dict(self, state):
        if tuple(state["thetas"].shape) != tuple(self.thetas.shape):
            raise ValueError("checkpoint holds %d agents, engine %d"
                             % (state["thetas"].shape[0],
                                self.thetas.shape[0]))
        if tuple(state["archive"].shape) != tuple(self.archive.shape):
            raise ValueError("checkpoint archive capacity %d, engine %d"
                             % (state["archive"].shape[0],
                                self.archive.shape[0]))
        self.thetas.copy_(state["thetas"].to(self.device))
        self.adam_m.copy_(state["adam_m"].to(self.device))
        self.adam_v.copy_(state["adam_v"].to(self.device))
        self.t_steps = [int(t) for t in state["t_steps"]]
        self.iteration = int(state["iteration"])
        self.obs_sum.copy_(state["obs_sum"].to(self.device))
        self.obs_sumsq.copy_(state["obs_sumsq"].to(self.device))
        self.obs_count.copy_(state["obs_count"].to(self.device))
        count = self.obs_count.clamp_min(1.0)
        self.obs_mu = (self.obs_sum / count).contiguous()
        var = self.obs_sumsq / count - self.obs_mu ** 2
        self.obs_nu = var.clamp_min(1e-2).contiguous()
        self.archive.copy_(state["archive"].to(self.device))
        self.archive_total = int(state["archive_total"])
        self.agent_bc.copy_(state["agent_bc"].to(self.device))
        self.weight = float(state["weight"])
        self.best_score = float(state["best_score"])
        self.stall = int(state["stall"])
        self._gen.set_state(state["generator"])

    def save(self, path):
        torch.save(self.state_dict(), path)

    def load(self, path):
        self.load_state_dict(torch.load(path, weights_only=False))
