"""A population of independent ES problems advanced together.

A POET population is P (policy, environment) pairs, each a small ES
problem of its own: its own theta, obs normaliser, Adam moments,
environment and noise stream.  ``ESEngine`` advances one of them per
``step()``: some eight small launches, three allocations and three host
syncs for a rollout that fills a fraction of the chip.  ``ESPopulation``
holds the state of all P stacked and advances them with one batched
rollout, rank and gradient launch each and row-wise Adam, without a host
sync.

Pair p computes exactly what ``ESEngine(replace(config, seed=seeds[p]),
env_params=env_params[p])`` computes: after any number of steps every
state tensor of row p equals that engine's bit for bit
(tests/gpu/test_es_population.py).  One GPU; sharding a population over
ranks is not covered.
"""

import dataclasses

import torch

from .. import ops, tracing
from .engine import ESConfig, init_theta

# per-pair state rows that travel with a policy in a transfer
_POLICY_FIELDS = ("theta", "obs_sum", "obs_sumsq", "obs_count", "obs_mu",
                  "obs_nu")
_STATE_FIELDS = ("theta", "adam_m", "adam_v", "obs_sum", "obs_sumsq",
                 "obs_count")


def _normaliser(obs_sum, obs_sumsq, obs_count):
    """(obs_mu, obs_nu) from the running sums: ESEngine's formulas, row-wise
    (obs_count is [P][1] and broadcasts over the 4 dims)."""
    count = obs_count.clamp_min(1.0)
    obs_mu = (obs_sum / count).contiguous()
    var = obs_sumsq / count - obs_mu ** 2
    return obs_mu, var.clamp_min(1e-2).contiguous()


class ESPopulation:
    def __init__(self, config: ESConfig, seeds, env_params, device=None):
        """``seeds``: P ints, pair p's noise stream and initial policy
        (``config.seed`` is not used).  ``env_params``: P tuples
        ``(env_A[4][4], env_B[4])``.  ``config.pop_per_gpu`` is the ES
        population of every pair."""
        self.cfg = config
        if device is None:
            device = torch.device("cuda", 0)
        self.device = device
        if config.pop_per_gpu % 2:
            raise ValueError("pop_per_gpu must be even (antithetic pairs)")
        self.seeds = [int(s) for s in seeds]
        P = self.P = len(self.seeds)
        if P < 1:
            raise ValueError("ESPopulation needs at least one pair")
        if len(env_params) != P:
            raise ValueError("%d seeds but %d env_params"
                             % (P, len(env_params)))
        n = config.obs_dim

        self._seeds_dev = ops.pair_seeds(self.seeds, device)
        self.theta = torch.stack(
            [init_theta(s, "cpu") for s in self.seeds]).to(device)
        self.adam_m = torch.zeros_like(self.theta)
        self.adam_v = torch.zeros_like(self.theta)
        self.t_step = 0  # shared: the pairs step together

        self.env_A = torch.empty(P, n, n, device=device)
        self.env_B = torch.empty(P, n, device=device)
        for p, (env_A, env_B) in enumerate(env_params):
            self.set_env(p, env_A, env_B)
        self.obs_sum = torch.zeros(P, n, device=device)
        self.obs_sumsq = torch.zeros(P, n, device=device)
        self.obs_count = torch.zeros(P, 1, device=device)
        self.obs_mu = torch.zeros(P, n, device=device)
        self.obs_nu = torch.ones(P, n, device=device)

    def __len__(self):
        return self.P

    # -- one ES iteration of every pair -----------------------------------
    def step(self, iteration=None):
        """ESEngine.step() for all pairs at once.  Returns device tensors
        of shape [P] (``fitness_mean``, ``fitness_max``, ``grad_norm``) and
        the two counts as ints; nothing here waits for the device."""
        cfg = self.cfg
        if iteration is None:
            iteration = self.t_step
        pop = cfg.pop_per_gpu

        with tracing.range("espop.rollout"):
            fitness, obs_stat = ops.es_rollout_mlp_pairs(
                self.theta, cfg.sigma, self._seeds_dev, iteration,
                cfg.horizon, pop, self.obs_mu, self.obs_nu, self.env_A,
                self.env_B)
        ranks = ops.centered_rank_pairs(fitness)
        wpair = (ranks[:, 0::2] - ranks[:, 1::2]).contiguous()
        with tracing.range("espop.grad"):
            grad = ops.es_grad_pairs(wpair, self._seeds_dev, iteration)
        grad /= float(pop) * cfg.sigma

        # maximize fitness => ascend; the same elementwise formulas as the
        # engine, on [P][NPARAMS]
        self.t_step += 1
        b1, b2 = cfg.adam_beta1, cfg.adam_beta2
        self.adam_m.mul_(b1).add_(grad, alpha=1 - b1)
        self.adam_v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
        mhat = self.adam_m / (1 - b1 ** self.t_step)
        vhat = self.adam_v / (1 - b2 ** self.t_step)
        self.theta.add_(cfg.lr * mhat / (vhat.sqrt() + cfg.adam_eps))

        # running obs normalization (applied next iteration)
        n = cfg.obs_dim
        self.obs_sum += obs_stat[:, :n]
        self.obs_sumsq += obs_stat[:, n:2 * n]
        self.obs_count += obs_stat[:, 2 * n:]
        self.obs_mu, self.obs_nu = _normaliser(self.obs_sum, self.obs_sumsq,
                                               self.obs_count)

        return {
            "fitness_mean": fitness.mean(dim=1),
            "fitness_max": fitness.max(dim=1).values,
            "grad_norm": grad.norm(dim=1),
            "rollouts": self.P * pop * cfg.envs_per_member,
            "env_steps": self.P * pop * cfg.envs_per_member * cfg.horizon,
        }

    # -- POET transfer step -------------------------------------------------
    def transfer_matrix(self, horizon, seed, iteration):
        """scores[P][P]: row k is pair k's current theta with its own obs
        normaliser, column m is pair m's environment.  One es_eval_matrix
        launch on the stacked state as it is, nothing is gathered."""
        return ops.es_eval_matrix(self.theta, self.obs_mu, self.obs_nu,
                                  self.env_A, self.env_B, seed, iteration,
                                  horizon)

    def apply_transfers(self, transfers):
        """For every ``(m, k)`` pair m takes the policy of pair k: theta
        and the obs statistics are copied and m's Adam moments zeroed.
        All donors are read from the pre-transfer state, as in
        ``poet.apply_transfers``; ``t_step`` and the environments stay."""
        last = {}
        for m, k in transfers:  # a repeated m: the last one wins
            if not (0 <= m < self.P and 0 <= k < self.P):
                raise IndexError("transfer (%d, %d) outside 0..%d"
                                 % (m, k, self.P - 1))
            last[m] = k
        if not last:
            return
        dst = torch.tensor(list(last.keys()), device=self.device)
        src = torch.tensor(list(last.values()), device=self.device)
        for name in _POLICY_FIELDS:
            field = getattr(self, name)
            field[dst] = field[src]  # the gather is a copy of the donors
        self.adam_m[dst] = 0.0
        self.adam_v[dst] = 0.0

    # -- POET reproduction: the population grows and shrinks ---------------
    _ROW_FIELDS = _STATE_FIELDS + ("obs_mu", "obs_nu", "env_A", "env_B")

    def add_pairs(self, seeds, env_params, donors):
        """Append ``len(seeds)`` pairs.  New pair i takes the policy rows
        (theta and the obs statistics) of existing pair ``donors[i]``, read
        from the state before the call, with zero Adam moments, its own
        seed (noise stream) ``seeds[i]`` and environment ``env_params[i]``
        = ``(env_A, env_B)``.  ``t_step`` stays shared, as in
        ``apply_transfers``.  From here on the new pair is, bit for bit,
        an ``ESEngine(replace(cfg, seed=seeds[i]), env_params=...)`` loaded
        with the donor's ``engine_state`` and the moments zeroed."""
        seeds = [int(s) for s in seeds]
        donors = [int(d) for d in donors]
        env_params = list(env_params)
        if not (len(seeds) == len(env_params) == len(donors)):
            raise ValueError("%d seeds, %d env_params, %d donors"
                             % (len(seeds), len(env_params), len(donors)))
        for d in donors:
            if not 0 <= d < self.P:
                raise IndexError("donor %d outside 0..%d" % (d, self.P - 1))
        n = self.cfg.obs_dim
        for env_A, env_B in env_params:
            if tuple(env_A.shape) != (n, n) or tuple(env_B.shape) != (n,):
                raise ValueError(
                    "env_params must be (env_A[%d][%d], env_B[%d])"
                    % (n, n, n))
        if not seeds:
            return
        src = torch.tensor(donors, device=self.device)
        for name in _POLICY_FIELDS:
            field = getattr(self, name)
            setattr(self, name, torch.cat([field, field[src]]).contiguous())
        for name in ("adam_m", "adam_v"):
            field = getattr(self, name)
            zeros = field.new_zeros((len(seeds),) + tuple(field.shape[1:]))
            setattr(self, name, torch.cat([field, zeros]).contiguous())
        new_A = torch.stack([a.detach().to(torch.float32)
                             for a, _b in env_params]).to(self.device)
        new_B = torch.stack([b.detach().to(torch.float32)
                             for _a, b in env_params]).to(self.device)
        self.env_A = torch.cat([self.env_A, new_A]).contiguous()
        self.env_B = torch.cat([self.env_B, new_B]).contiguous()
        self._set_seeds(self.seeds + seeds)

    def remove_pairs(self, indices):
        """Drop the pairs ``indices`` (the others keep their order and
        every bit of their state).  Returns ``(env_A[R][4][4],
        env_B[R][4], seeds)`` of the removed pairs in ascending index
        order, for the caller's archive."""
        drop = sorted({int(i) for i in indices})
        for i in drop:
            if not 0 <= i < self.P:
                raise IndexError("pair %d outside 0..%d" % (i, self.P - 1))
        if len(drop) >= self.P:
            raise ValueError("remove_pairs would leave no pair")
        gone = set(drop)
        keep = [p for p in range(self.P) if p not in gone]
        drop_idx = torch.tensor(drop, dtype=torch.long, device=self.device)
        keep_idx = torch.tensor(keep, dtype=torch.long, device=self.device)
        removed = (self.env_A[drop_idx], self.env_B[drop_idx],
                   [self.seeds[i] for i in drop])
        if drop:
            for name in self._ROW_FIELDS:
                setattr(self, name,
                        getattr(self, name)[keep_idx].contiguous())
            self._set_seeds([self.seeds[p] for p in keep])
        return removed

    def _set_seeds(self, seeds):
        self.seeds = list(seeds)
        self.P = len(self.seeds)
        self._seeds_dev = ops.pair_seeds(self.seeds, self.device)

    def set_env(self, p, env_A, env_B):
        """Replace pair p's environment (copies, like ESEngine)."""
        n = self.cfg.obs_dim
        if tuple(env_A.shape) != (n, n) or tuple(env_B.shape) != (n,):
            raise ValueError("env_params must be (env_A[%d][%d], env_B[%d])"
                             % (n, n, n))
        self.env_A[p].copy_(env_A.detach().to(torch.float32))
        self.env_B[p].copy_(env_B.detach().to(torch.float32))

    # -- checkpoint / lifting a pair out -------------------------------------
    def engine_state(self, p):
        """Pair p as a dict that ``ESEngine.load_state_dict`` accepts; the
        engine it is loaded into is built with ``seed=seeds[p]`` and pair
        p's environment (``env_A[p]``, ``env_B[p]``)."""
        state = {f: getattr(self, f)[p].cpu() for f in _STATE_FIELDS}
        state["t_step"] = self.t_step
        state["config"] = dataclasses.asdict(
            dataclasses.replace(self.cfg, seed=self.seeds[p]))
        return state

    def state_dict(self):
        """The whole population.  Unlike an engine's, it includes the
        environments: they are what makes the pairs differ."""
        state = {f: getattr(self, f).cpu() for f in _STATE_FIELDS}
        state.update({
            "t_step": self.t_step,
            "seeds": list(self.seeds),
            "env_A": self.env_A.cpu(),
            "env_B": self.env_B.cpu(),
            "config": dataclasses.asdict(self.cfg),
        })
        return state

    def load_state_dict(self, state):
        if list(state["seeds"]) != self.seeds:
            raise ValueError("state_dict is for seeds %s, population has %s"
                             % (list(state["seeds"]), self.seeds))
        for f in _STATE_FIELDS + ("env_A", "env_B"):
            getattr(self, f).copy_(state[f].to(self.device))
        self.t_step = int(state["t_step"])
        self.obs_mu, self.obs_nu = _normaliser(self.obs_sum, self.obs_sumsq,
                                               self.obs_count)
