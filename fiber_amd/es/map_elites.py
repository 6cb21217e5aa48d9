"""MAP-Elites on the MLP engine: the quality-diversity line of deep
neuroevolution (Mouret & Clune, "Illuminating search spaces by mapping
elites").

The archive is a grid over behaviour space with one elite per cell.  The
behaviour characterisation (BC) of a policy is the one the novelty-seeking
engines use: the mean final state over its 64 episodes, 4 floats.  Each
generation mutates elites drawn uniformly from the filled cells, as the Deep
GA mutates its survivors, and a child replaces the occupant of the cell its
BC falls in only if it is strictly fitter.  The result is a map of the best
policy found for each kind of behaviour, not one champion.

The grid has ``bins[d]`` bins over ``[bc_lo[d], bc_hi[d])`` in dimension d
(``bins[d] = 1`` ignores a dimension) and ``C = prod(bins)`` cells; BCs
outside the bounds clamp to the edge cells.  The state, all on the device:
``theta0 = init_theta(seed)``; the weights ``arch_theta[C + 1][NPARAMS]``,
row C the root ``theta0``, never replaced, and rows of empty cells ``theta0``
too; ``arch_fitness[C]``, ``arch_bc[C][4]``, ``arch_filled[C]`` (int32) and
``arch_born[C]`` (the generation that inserted the occupant, -1 for none);
the seed chains ``lineage[C + 1][cap]`` in ``ga_decode``'s format (the root
row all -1, the capacity doubles when full); the compact list ``filled_idx[C]``
with its length ``n_filled[1]``; ``generation`` and ``ESEngine``'s obs
normaliser.  One generation is:

  1. me_parents         — member m mutates the elite of a drawn filled cell
                          (the root while the archive is empty) with the draw
                          of slot m; the number of filled cells is read on
                          the device
  2. ga_rollout_mlp_bc  — ONE launch: fitness, obs statistics and BC
  3. me_insert          — cell of every member, the per-cell competition by
                          a 64-bit atomic maximum, the archive's fitness, BC
                          and filled flags
  4. ga_survivors       — the archive's weights, out of place into the other
                          half of a double buffer: a new elite's parent may
                          be replaced in the same generation
  5. lineage gather     — torch indexing, as in GAEngine.step
  6. me_compact         — the filled cells, compact and ascending
  7. obs-normaliser merge — ESEngine.step's lines

Generation g uses the draws and start states of ``(seed, g)``, as the GA
does.  If ``bc_lo`` / ``bc_hi`` are None they are fixed once, on the host,
after generation 0's rollout and before its insert: per dimension the
minimum and maximum of that generation's finite BCs, widened by half the
range on each side (by 1 if the range is 0).  That is the one host sync the
kernels of a run need; they are then stored and checkpointed.

``arch_theta`` is a cache of ``ga_decode(theta0, lineage)``, which rebuilds
it bit for bit; a checkpoint stores the chains and not the weights.

Stated limits.  An elite's stored fitness and BC are those measured when it
was inserted, with that generation's start states and obs normaliser: elites
are not re-scored.  Parent choice is uniform over the filled cells.  Sigma is
one constant scalar.  MLP engine only (no conv engine, no ``ESPopulation``),
single process.
"""

import dataclasses
import math

import numpy as np
import torch

from .. import ops, tracing
from .engine import init_theta, make_env_params


@dataclasses.dataclass
class MapElitesConfig:
    pop: int = 1024
    bins: tuple = (8, 8, 1, 1)    # bins per BC dimension; 1 ignores it
    bc_lo: tuple = None           # 4 floats, or None: fixed after generation 0
    bc_hi: tuple = None
    sigma: float = 0.02           # mutation step, constant
    horizon: int = 200
    seed: int = 1234
    # fixed by the compiled kernel:
    obs_dim: int = ops.OBS_DIM
    envs_per_member: int = ops.ENVS_PER_MEMBER

    def __post_init__(self):
        self.validate()

    @property
    def cells(self):
        C = 1
        for b in self.bins:
            C *= int(b)
        return C

    def validate(self):
        """ValueError unless 1 <= pop <= 65536, bins is 4 ints >= 1 with at
        most ME_CELLS_MAX cells, bc_lo and bc_hi are both None or both 4
        finite floats with hi > lo, horizon >= 1 and sigma finite and
        >= 0."""
        if not 1 <= self.pop <= ops.GA_TRUNCATE_MAX:
            raise ValueError("pop must be in [1, %d], got %r"
                             % (ops.GA_TRUNCATE_MAX, self.pop))
        try:
            bins = tuple(self.bins)
        except TypeError:
            raise ValueError("bins must be 4 ints, got %r" % (self.bins,))
        if len(bins) != ops.BC_DIM or any(
                int(b) != b or b < 1 for b in bins):
            raise ValueError("bins must be %d ints >= 1, got %r"
                             % (ops.BC_DIM, self.bins))
        self.bins = tuple(int(b) for b in bins)
        if self.cells + 1 > ops.GA_ROWS_MAX:
            raise ValueError("bins %r give %d cells, more than %d"
                             % (self.bins, self.cells, ops.ME_CELLS_MAX))
        if (self.bc_lo is None) != (self.bc_hi is None):
            raise ValueError("bc_lo and bc_hi must both be given or both be "
                             "None")
        if self.bc_lo is not None:
            self.bc_lo = tuple(float(x) for x in self.bc_lo)
            self.bc_hi = tuple(float(x) for x in self.bc_hi)
            ops.me_grid(self.bins, self.bc_lo, self.bc_hi)
        if self.horizon < 1:
            raise ValueError("horizon must be >= 1, got %r" % self.horizon)
        if not 0.0 <= self.sigma < math.inf:  # also refuses a NaN
            raise ValueError("sigma must be finite and >= 0, got %r"
                             % self.sigma)


def bounds_from_bc(bc):
    """The bounds fixed after generation 0: per dimension the minimum and
    maximum over the rows of ``bc[pop][4]`` (numpy) that are finite
    throughout, widened by half the range on each side, by 1 where the range
    is 0; (-1, 1) with no finite row.  Two tuples of 4 Python floats."""
    bc = np.asarray(bc, dtype=np.float64).reshape(-1, ops.BC_DIM)
    rows = bc[np.isfinite(bc).all(axis=1)]
    if rows.shape[0] == 0:
        rows = np.zeros((1, ops.BC_DIM))
    lo, hi = rows.min(axis=0), rows.max(axis=0)
    pad = np.where(hi > lo, (hi - lo) / 2, 1.0)
    return (tuple(float(x) for x in lo - pad),
            tuple(float(x) for x in hi + pad))


class MapElitesEngine:
    def __init__(self, config: MapElitesConfig, ctx=None, device=None,
                 env_params=None):
        if ctx is not None:
            raise NotImplementedError(
                "data-parallel MAP-Elites is not built yet: fitness and BC "
                "would have to be all-gathered before the insert; run "
                "MapElitesEngine in one process (ctx=None)")
        config.validate()
        self.cfg = config
        if device is None:
            device = torch.device("cuda", 0)
        self.device = device
        C = self.cells = config.cells
        pop = config.pop

        self.theta0 = init_theta(config.seed, device)
        # double buffer: ga_survivors writes the half that is not read
        self.arch_theta = self.theta0.repeat(C + 1, 1)
        self._spare_theta = torch.empty_like(self.arch_theta)
        self.arch_fitness = torch.zeros(C, device=device)
        self.arch_bc = torch.zeros(C, ops.BC_DIM, device=device)
        self.arch_filled = torch.zeros(C, dtype=torch.int32, device=device)
        self.arch_born = torch.full((C,), -1, dtype=torch.int32,
                                    device=device)
        self.lineage = torch.full((C + 1, 8), -1, dtype=torch.int32,
                                  device=device)
        self.filled_idx = torch.full((C,), -1, dtype=torch.int32,
                                     device=device)
        self.n_filled = torch.zeros(1, dtype=torch.int32, device=device)
        self.generation = 0
        self.bc_lo, self.bc_hi = config.bc_lo, config.bc_hi

        # parent_idx / slot of the members, followed by the C + 1
        # pseudo-members through which ga_survivors copies a row as it is:
        # pseudo-member pop + c has parent c and slot -1
        self._parent_ext = torch.cat([
            torch.zeros(pop, dtype=torch.int32, device=device),
            torch.arange(C + 1, dtype=torch.int32, device=device)])
        self._slot_ext = torch.full((pop + C + 1,), -1, dtype=torch.int32,
                                    device=device)

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

    # -- the best elite ------------------------------------------------------
    def best_cell(self):
        """The filled cell of greatest stored fitness (the lowest index among
        equals), or None while the archive is empty.  One host sync."""
        if int(self.n_filled) == 0:
            return None
        masked = torch.where(self.arch_filled != 0, self.arch_fitness,
                             torch.full_like(self.arch_fitness, -math.inf))
        best = masked.max()
        return int(torch.nonzero(
            (masked == best) & (self.arch_filled != 0))[0])

    @property
    def theta(self):
        """The weights of the best elite (theta0 before the first step)."""
        c = self.best_cell()
        return self.theta0 if c is None else self.arch_theta[c]

    # -- one generation ------------------------------------------------------
    def step(self):
        cfg = self.cfg
        g, C, pop = self.generation, self.cells, cfg.pop

        parent_idx, slot = ops.me_parents(
            cfg.seed, g, pop, self.filled_idx, self.n_filled, C,
            out_parent_idx=self._parent_ext[:pop],
            out_slot=self._slot_ext[:pop])
        with tracing.range("me.rollout"):
            fitness, obs_stat, bc = ops.ga_rollout_mlp_bc(
                self.arch_theta, parent_idx, slot, cfg.sigma, cfg.seed, g,
                cfg.horizon, self.obs_mu, self.obs_nu, self.env_A,
                self.env_B)
        if self.bc_lo is None:
            # the one host sync of a run: the grid is fixed from what
            # generation 0 did
            self.bc_lo, self.bc_hi = bounds_from_bc(bc.cpu().numpy())
        with tracing.range("me.insert"):
            cell, winner, order = ops.me_insert(
                fitness, bc, cfg.bins, self.bc_lo, self.bc_hi,
                self.arch_fitness, self.arch_bc, self.arch_filled)
        with tracing.range("me.materialise"):
            ops.ga_survivors(self.arch_theta, self._parent_ext,
                             self._slot_ext, order, cfg.sigma, cfg.seed, g,
                             out=self._spare_theta)
        self.arch_theta, self._spare_theta = (self._spare_theta,
                                              self.arch_theta)

        # seed chains of the archive's rows (plumbing: torch indexing)
        cap = self.lineage.shape[1]
        if g >= cap:
            cap *= 2
        chosen = order.long()
        lineage = torch.full((C + 1, cap), -1, dtype=torch.int32,
                             device=self.device)
        lineage[:, :g] = self.lineage[self._parent_ext[chosen].long(), :g]
        lineage[:, g] = self._slot_ext[chosen]
        self.lineage = lineage
        changed = winner >= 0
        self.arch_born = torch.where(
            changed, torch.full_like(self.arch_born, g), self.arch_born)

        ops.me_compact(self.arch_filled, out_filled_idx=self.filled_idx,
                       out_n_filled=self.n_filled)
        self.generation = g + 1
        # parent_idx and slot are views of buffers the next step rewrites
        self.last = {"fitness": fitness, "bc": bc, "cell": cell,
                     "winner": winner, "parent_idx": parent_idx.clone(),
                     "slot": slot.clone()}

        # running obs normalization (applied next generation)
        self.obs_sum += obs_stat[: cfg.obs_dim]
        self.obs_sumsq += obs_stat[cfg.obs_dim : 2 * cfg.obs_dim]
        self.obs_count += obs_stat[2 * cfg.obs_dim]
        count = self.obs_count.clamp_min(1.0)
        self.obs_mu = (self.obs_sum / count).contiguous()
        var = self.obs_sumsq / count - self.obs_mu ** 2
        self.obs_nu = var.clamp_min(1e-2).contiguous()

        on = self.arch_filled != 0
        n_filled = int(self.n_filled)
        held = torch.where(on, self.arch_fitness,
                           torch.zeros_like(self.arch_fitness))
        return {
            "coverage": n_filled / C,
            # sum of the stored fitness over the filled cells
            "qd_score": float(held.sum()),
            "fitness_max": float(self.arch_fitness[on].max()) if n_filled
            else float("nan"),
            "inserted": int(changed.sum()),
            "rollouts": pop * cfg.envs_per_member,
            "env_steps": pop * cfg.envs_per_member * cfg.horizon,
            "generation": self.generation,   # generations completed
        }

    # -- score the best elite ------------------------------------------------
    def evaluate(self, horizon=None, iteration=None, return_episodes=False):
        """Mean return of ``theta``, unmutated, on this engine's environment
        with its current obs normaliser: one es_eval_matrix launch with K =
        M = 1, as GAEngine.evaluate.  The 64 episodes start from the states
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

    # -- the archive, cell by cell ---------------------------------------------
    def _check_cell(self, cell):
        cell = int(cell)
        if not 0 <= cell < self.cells:
            raise IndexError("cell %r of %d" % (cell, self.cells))
        if not int(self.arch_filled[cell]):
            raise KeyError("cell %d is empty" % cell)
        return cell

    def genome(self, cell):
        """The seed chain of the elite of ``cell``: an int32 CPU tensor
        [generation], entry c the child slot whose draw was applied in
        generation c, or -1.  IndexError outside the grid, KeyError for an
        empty cell."""
        cell = self._check_cell(cell)
        return self.lineage[cell, : self.generation].cpu()

    def elite(self, cell):
        """``(theta, fitness, bc, genome)`` of the elite of ``cell``: its
        weights (a device row), the fitness and the BC (CPU tensor [4]) it
        was inserted with, and its seed chain."""
        cell = self._check_cell(cell)
        return (self.arch_theta[cell], float(self.arch_fitness[cell]),
                self.arch_bc[cell].cpu(), self.genome(cell))

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
        """theta0, the seed chains, the archive's fitness, BC, filled flags
        and birth generations, the bounds, the obs sums and the config; not
        the weights, which load_state_dict() decodes again."""
        return {
            "theta0": self.theta0.cpu(),
            "me_lineage": self.lineage[:, : self.generation].cpu(),
            "arch_fitness": self.arch_fitness.cpu(),
            "arch_bc": self.arch_bc.cpu(),
            "arch_filled": self.arch_filled.cpu(),
            "arch_born": self.arch_born.cpu(),
            "bc_lo": self.bc_lo,
            "bc_hi": self.bc_hi,
            "generation": self.generation,
            "obs_sum": self.obs_sum.cpu(),
            "obs_sumsq": self.obs_sumsq.cpu(),
            "obs_count": self.obs_count.cpu(),
            "config": dataclasses.asdict(self.cfg),
        }

    def load_state_dict(self, state):
        """Rebuild ``arch_theta`` from the saved chains with ga_decode and
        the list of filled cells with me_compact.  The checkpoint's sigma,
        seed and bins must be this engine's (ValueError otherwise): the
        chains mean nothing under other draws, the archive nothing on
        another grid.  pop and horizon are not compared.  The bounds are the
        checkpoint's."""
        if "me_lineage" not in state or "theta0" not in state:
            raise ValueError("the checkpoint holds no archive: it is not a "
                             "MapElitesEngine's")
        saved = state["config"]
        for key in ("sigma", "seed", "bins"):
            mine = getattr(self.cfg, key)
            theirs = saved[key]
            if key == "bins":
                mine, theirs = tuple(mine), tuple(theirs)
            if theirs != mine:
                raise ValueError("the checkpoint was written with %s = %r, "
                                 "this engine has %r" % (key, theirs, mine))
        C = self.cells
        generation = int(state["generation"])
        lineage = state["me_lineage"]
        if tuple(lineage.shape) != (C + 1, generation):
            raise ValueError("checkpoint lineage has shape %s at generation "
                             "%d with %d cells"
                             % (tuple(lineage.shape), generation, C))
        if tuple(state["theta0"].shape) != tuple(self.theta0.shape):
            raise ValueError("checkpoint theta0 has shape %s"
                             % (tuple(state["theta0"].shape),))
        for name, want in (("arch_fitness", (C,)),
                           ("arch_bc", (C, ops.BC_DIM)),
                           ("arch_filled", (C,)), ("arch_born", (C,))):
            if tuple(state[name].shape) != want:
                raise ValueError("checkpoint %s has shape %s"
                                 % (name, tuple(state[name].shape)))
        if (state["bc_lo"] is None) != (state["bc_hi"] is None) or (
                state["bc_lo"] is None and generation > 0):
            raise ValueError("the checkpoint holds no bounds")
        if state["bc_lo"] is not None:
            ops.me_grid(self.cfg.bins, state["bc_lo"], state["bc_hi"])
        self.theta0.copy_(state["theta0"].to(self.device))
        rows = lineage.to(device=self.device, dtype=torch.int32).contiguous()
        ops.ga_decode(self.theta0, rows, self.cfg.sigma, self.cfg.seed,
                      out=self.arch_theta)
        cap = 8
        while cap < generation:
            cap *= 2
        self.lineage = torch.full((C + 1, cap), -1, dtype=torch.int32,
                                  device=self.device)
        self.lineage[:, :generation] = rows
        self.arch_fitness.copy_(state["arch_fitness"].to(self.device))
        self.arch_bc.copy_(state["arch_bc"].to(self.device))
        self.arch_filled.copy_(state["arch_filled"].to(self.device))
        self.arch_born.copy_(state["arch_born"].to(self.device))
        ops.me_compact(self.arch_filled, out_filled_idx=self.filled_idx,
                       out_n_filled=self.n_filled)
        self.bc_lo = None if state["bc_lo"] is None \
            else tuple(float(x) for x in state["bc_lo"])
        self.bc_hi = None if state["bc_hi"] is None \
            else tuple(float(x) for x in state["bc_hi"])
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
