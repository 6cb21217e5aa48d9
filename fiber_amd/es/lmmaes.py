"""LM-MA-ES on the MLP engine: the limited-memory matrix adaptation
evolution strategy (Loshchilov, Glasmachers, Beyer, "Large Scale Black-box
Optimization by Limited-Memory Matrix Adaptation", 2019), the member of the
CMA family that fits the "nothing materialised" style of this package.  It
learns correlations between parameters through m = 29 direction vectors and
adapts the global step size; every other scalar-sigma engine here samples
from a fixed isotropic Gaussian.

The state is ``theta[n]``, the scalar ``sigma`` (a Python float, starting at
``config.sigma``), ``p_sigma[n]``, ``dirs[m][n]`` (the paper's m_i, zero at
the start) and ``t_step``.  With n = NPARAMS, lambda = ``pop_per_gpu``, mu =
lambda / 2 and J = min(t_step, m) active directions, one iteration is:

  1. es_rollout_mlp_lowrank — member 2k evaluates theta + sigma * d_k and
                              member 2k+1 theta - sigma * d_k, d_k = T z_k,
                              z_k the draw es_rollout_mlp gives pair k, T
                              the paper's chain d <- (1 - c_d[j]) d +
                              c_d[j] m_j (m_j . d), j = 1 .. J
  2. centered_rank          — distinct ranks with a fixed tie order; the
                              member at position i (1 is the best) gets w_i
                              = max(0, ln(mu + 1/2) - ln i), normalised to
                              sum 1; mu_w = 1 / sum w_i^2; wpair[k] =
                              w(member 2k) - w(member 2k+1)
  3. es_grad(wpair)         — g_z = sum_i w_i z_i, the draws regenerated
  4. g_d = T g_z            — one vector, because T is linear
  5. theta   += lr_mean * sigma * g_d
     p_sigma  = (1 - c_sigma) p_sigma + sqrt(mu_w c_sigma (2 - c_sigma)) g_z
     dirs[i]  = (1 - c_c[i]) dirs[i] + sqrt(mu_w c_c[i] (2 - c_c[i])) g_z
     sigma   *= exp((c_sigma / 2) (|p_sigma|^2 / n - 1)), clamped to
                [sigma_min, sigma_max]
     The first three read the values from before the step; sigma reads the
     new p_sigma, as in the paper.
  6. obs-normaliser merge   — ESEngine.step's lines

The kernel does not run the chain, which is J block-wide dot products one
after the other.  With d_j = a_j z + sum_{k<=j} b_{j,k} m_k, p = M z and G =
M M^t (M the J active rows), the chain's dot product is s_j = a_{j-1} p_j +
sum_{k<j} b_{j-1,k} G[k][j], so b is linear in p and

    T = a I + M^t L M,   a = prod_j (1 - c_d[j]),   L lower triangular.

``sampling_mix`` forms (a, L) once per iteration from the J x J Gram matrix,
in float64; the kernel needs one pass over M for all dot products, one
block reduction, and a second pass (lowrank_kernels.hip).

The rates are the paper's, all overridable and all untuned here: m = 4 +
floor(3 ln n) = 29, c_sigma = 2 lambda_0 / n, c_d[i] = 1 / (1.5^i n),
c_c[i] = lambda_0 / (4^i n) for i = 0 .. m-1, with lambda_0 = 4 + floor(3
ln n) the paper's default population and NOT the run's: the formulas
assume lambda << n, and at this package's populations (up to 32768 > n)
they would exceed 1.  ``sigma_min = 1e-3 * config.sigma`` and ``sigma_max =
10 * config.sigma`` are guard rails like SNESConfig's.

Limits: the 64-wide MLP policy on the linear environment, one process (no
ring context).  No CartPole, recurrent, wide or POET variant.
"""

import dataclasses
import math

import numpy as np
import torch

from .. import ops, tracing
from . import _core
from .engine import ESConfig, ESEngine, init_theta


def default_n_dirs(nparams=ops.NPARAMS):
    """4 + floor(3 ln n), the paper's m and its default population."""
    return 4 + int(math.floor(3.0 * math.log(nparams)))


def recombination_weights(pop):
    """``(w, mu_w)``: ``w[i - 1] = max(0, ln(mu + 1/2) - ln i)`` for the
    positions i = 1 .. pop (1 is the best), mu = pop / 2, normalised to sum
    1, as a float64 CPU tensor; ``mu_w = 1 / sum w^2``."""
    i = torch.arange(1, pop + 1, dtype=torch.float64)
    w = (math.log(pop // 2 + 0.5) - torch.log(i)).clamp_min(0.0)
    w /= w.sum()
    return w, 1.0 / float((w * w).sum())


def pair_weights(ranks, w_table):
    """``wpair[k] = w(member 2k) - w(member 2k+1)`` from the centered ranks
    of the population (``ops.centered_rank``: r / (pop - 1) - 0.5 with r = 0
    the worst) and the per-position table on the same device: the member of
    rank r sits at position pop - r."""
    pop = ranks.numel()
    r = torch.round((ranks + 0.5) * (pop - 1)).long()
    w = w_table[pop - 1 - r]
    return (w[0::2] - w[1::2]).contiguous()


@dataclasses.dataclass
class LMMAESConfig:
    # None: the paper's value, see the module docstring.  Untuned here.
    n_dirs: int = None
    c_sigma: float = None
    c_d: list = None      # [n_dirs]
    c_c: list = None      # [n_dirs]
    lr_mean: float = 1.0
    sigma_min: float = None
    sigma_max: float = None

    def resolved(self, config: ESConfig):
        """A copy with every None replaced by its default for ``config``."""
        n, lam0 = ops.NPARAMS, default_n_dirs()
        m = lam0 if self.n_dirs is None else int(self.n_dirs)
        c_sigma = 2.0 * lam0 / n
        c_d = [1.0 / (1.5 ** i * n) for i in range(m)]
        c_c = [lam0 / (4.0 ** i * n) for i in range(m)]
        return LMMAESConfig(
            n_dirs=m,
            c_sigma=float(c_sigma if self.c_sigma is None else self.c_sigma),
            c_d=[float(c) for c in (c_d if self.c_d is None else self.c_d)],
            c_c=[float(c) for c in (c_c if self.c_c is None else self.c_c)],
            lr_mean=float(self.lr_mean),
            sigma_min=(1e-3 * config.sigma if self.sigma_min is None
                       else float(self.sigma_min)),
            sigma_max=(10.0 * config.sigma if self.sigma_max is None
                       else float(self.sigma_max)))


def mix_from_gram(G, c_d):
    """``(a, L)`` of T = a I + M^t L M from the Gram matrix ``G = M M^t``
    and the rates of the J active directions, float64 numpy.  Row k of L
    holds b_k as a combination of p = M z; it is lower triangular."""
    J = len(c_d)
    a = 1.0
    L = np.zeros((J, J))
    for j in range(J):
        s = G[:j, j] @ L[:j]      # s_j as a combination of p
        s[j] += a
        a *= 1.0 - c_d[j]
        L[:j] *= 1.0 - c_d[j]
        L[j] = c_d[j] * s
    return a, L


def sampling_mix(dirs, c_d):
    """``(scale, mix)`` for the kernels' ``scale * I + dirs^t mix dirs``,
    equal to the paper's chain over the rows of ``dirs[J][n]`` with the
    rates ``c_d[J]``.  The Gram matrix is one float64 matmul on the device
    of ``dirs``, the recurrence runs on the host.  ``mix`` is a float64
    ``[J][J]`` lower triangle on that device."""
    J = dirs.shape[0]
    if len(c_d) != J:
        raise ValueError("%d rates for %d directions" % (len(c_d), J))
    M = dirs.double()
    a, L = mix_from_gram((M @ M.T).cpu().numpy(), c_d)
    return a, torch.from_numpy(L).to(dirs.device)


class LMMAESEngine(_core.ObsNormaliser):
    def __init__(self, config: ESConfig, lmmaes: LMMAESConfig = None,
                 ctx=None, device=None, env_params=None):
        if ctx is not None:
            raise NotImplementedError(
                "data-parallel LM-MA-ES is not built yet: run LMMAESEngine "
                "in one process (ctx=None)")
        lm = (lmmaes or LMMAESConfig()).resolved(config)
        m = lm.n_dirs
        if not 1 <= m <= ops.LOWRANK_DIRS_MAX:
            raise ValueError("n_dirs must be in [1, %d], got %d"
                             % (ops.LOWRANK_DIRS_MAX, m))
        if len(lm.c_d) != m or len(lm.c_c) != m:
            raise ValueError("c_d and c_c must hold n_dirs = %d rates" % m)
        if not all(0.0 < c < 1.0 for c in [lm.c_sigma] + lm.c_d + lm.c_c):
            raise ValueError("c_sigma, c_d and c_c must lie in (0, 1)")
        if not 0.0 < lm.sigma_min <= lm.sigma_max < math.inf:
            raise ValueError("need 0 < sigma_min <= sigma_max < inf, got "
                             "%r, %r" % (lm.sigma_min, lm.sigma_max))
        if config.pop_per_gpu % 2 or config.pop_per_gpu < 2:
            raise ValueError("pop_per_gpu must be even (antithetic pairs)")
        self.cfg, self.lm = config, lm
        if device is None:
            device = torch.device("cuda", 0)
        self.device = device
        self.pop_total = config.pop_per_gpu

        self.theta = init_theta(config.seed, device)
        self.sigma = float(config.sigma)
        self.p_sigma = torch.zeros_like(self.theta)
        self.dirs = torch.zeros(m, ops.NPARAMS, device=device)
        self.t_step = 0
        self.env_A, self.env_B = _core.resolve_env(config, device,
                                                   env_params)
        self._init_normaliser()

        # per-position weights (float64 on the host, one rounding to fp32)
        # and the update's coefficients
        w, self._mu_w = recombination_weights(self.pop_total)
        self._w_table = w.float().to(device)
        c_c = np.asarray(lm.c_c)
        col = dict(dtype=torch.float32, device=device)
        self._dir_decay = torch.tensor(1.0 - c_c, **col).unsqueeze(1)
        self._dir_coef = torch.tensor(
            np.sqrt(self._mu_w * c_c * (2.0 - c_c)), **col).unsqueeze(1)

    # -- sampling ------------------------------------------------------------
    def sampling(self):
        """``(dirs[:J], scale, mix fp64)`` of the next step's population."""
        J = min(self.t_step, self.lm.n_dirs)
        active = self.dirs[:J]
        scale, mix = sampling_mix(active, self.lm.c_d[:J])
        return active, scale, mix

    def sample(self, k, iteration=None):
        """The parameters of members 0 .. k-1 as ``step(iteration)`` would
        roll them out: fp32 ``[k][NPARAMS]``.  Changes nothing."""
        if iteration is None:
            iteration = self.t_step
        active, scale, mix = self.sampling()
        return ops.es_perturb_lowrank(
            self.theta, self.sigma, active, mix.float().contiguous(), scale,
            self.cfg.seed, iteration, 0, k)

    # -- one LM-MA-ES iteration ------------------------------------------------
    def step(self, iteration=None):
        cfg, lm = self.cfg, self.lm
        if iteration is None:
            iteration = self.t_step
        pop = cfg.pop_per_gpu
        active, scale, mix = self.sampling()

        with tracing.range("lmmaes.rollout"):
            fitness, obs_stat = ops.es_rollout_mlp_lowrank(
                self.theta, self.sigma, active, mix.float().contiguous(),
                scale, cfg.seed, iteration, cfg.horizon, 0, pop, self.obs_mu,
                self.obs_nu, self.env_A, self.env_B)

        wpair = pair_weights(ops.centered_rank(fitness), self._w_table)

        with tracing.range("lmmaes.grad"):
            g_z = ops.es_grad(wpair, 0, pop // 2, cfg.seed, iteration,
                              self.device)
        # g_d = T g_z in float64, rounded once
        M = active.double()
        gz64 = g_z.double()
        g_d = (scale * gz64 + M.T @ (mix @ (M @ gz64))).float()

        self.theta.add_(g_d, alpha=lm.lr_mean * self.sigma)
        c_s = lm.c_sigma
        self.p_sigma.mul_(1.0 - c_s).add_(
            g_z, alpha=math.sqrt(self._mu_w * c_s * (2.0 - c_s)))
        self.dirs.mul_(self._dir_decay).add_(self._dir_coef * g_z)
        norm2 = float(self.p_sigma.double().square().sum())
        self.sigma = min(max(
            self.sigma * math.exp(0.5 * c_s * (norm2 / ops.NPARAMS - 1.0)),
            lm.sigma_min), lm.sigma_max)
        self.t_step += 1

        # running obs normalization (applied next iteration)
        self._merge_obs_stat(obs_stat)

        return {
            "fitness_mean": float(fitness.mean()),
            "fitness_max": float(fitness.max()),
            "grad_norm": float(g_d.norm()),
            "rollouts": pop * cfg.envs_per_member,
            "env_steps": pop * cfg.envs_per_member * cfg.horizon,
            "sigma": self.sigma,
            "n_active": active.shape[0],
        }

    # evaluate() and act() read theta, the normaliser and the environment
    # only: ESEngine's, as they are
    evaluate = ESEngine.evaluate
    act = ESEngine.act

    # -- checkpoint / resume ----------------------------------------------
    def state_dict(self):
        return {
            "theta": self.theta.cpu(),
            "t_step": self.t_step,
            **self._obs_state(),
            "sigma": self.sigma,
            "p_sigma": self.p_sigma.cpu(),
            "dirs": self.dirs.cpu(),
            "config": dataclasses.asdict(self.cfg),
            "lmmaes_config": dataclasses.asdict(self.lm),
        }

    def load_state_dict(self, state):
        if "dirs" not in state or "p_sigma" not in state:
            raise ValueError("the checkpoint holds no direction vectors: it "
                             "is not an LMMAESEngine's")
        if tuple(state["dirs"].shape) != tuple(self.dirs.shape):
            raise ValueError("checkpoint dirs has shape %s, engine %s"
                             % (tuple(state["dirs"].shape),
                                tuple(self.dirs.shape)))
        self.theta.copy_(state["theta"].to(self.device))
        self.t_step = int(state["t_step"])
        self._load_obs_state(state)
        self.sigma = float(state["sigma"])
        self.p_sigma.copy_(state["p_sigma"].to(self.device))
        self.dirs.copy_(state["dirs"].to(self.device))

    save, load = _core.save, _core.load
