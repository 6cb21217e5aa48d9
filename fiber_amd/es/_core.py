"""Host-side state and update shared by the ES engines.

Every engine in this package resolves its environment, keeps the running
observation normaliser, ascends with Adam, normalises ``act()`` input and
checkpoints in the same way.  Each of those is written here once; the fp64
oracles (update_oracle.py) model exactly these torch sequences, operation by
operation.

``RolloutESEngine`` is ``ESEngine``'s iteration for one GPU with the
rollout swapped: an engine built on it supplies ``_init_theta``,
``_rollout``, ``nparams`` and ``_range``.
"""

import torch

from .. import ops, tracing


# -- environment ------------------------------------------------------------
def make_env_params(seed, device):
    """Fixed synthetic-env dynamics, identical on every rank."""
    gen = torch.Generator().manual_seed(seed ^ 0xE17)
    env_A = (torch.randn(4, 4, generator=gen) * 0.5).to(device)
    env_B = torch.randn(4, generator=gen).to(device)
    return env_A.contiguous(), env_B.contiguous()


def check_env_shapes(env_A, env_B, n):
    if tuple(env_A.shape) != (n, n) or tuple(env_B.shape) != (n,):
        raise ValueError("env_params must be (env_A[%d][%d], env_B[%d])"
                         % (n, n, n))


def resolve_env(config, device, env_params):
    """``(env_A, env_B)`` of an engine.  ``env_params = (env_A[4][4],
    env_B[4])`` puts it on a given environment (a POET pair); None is the one
    derived from ``config.seed``.  The environment is not part of an engine's
    state_dict()."""
    if env_params is None:
        return make_env_params(config.seed, device)
    env_A, env_B = env_params
    check_env_shapes(env_A, env_B, config.obs_dim)
    # own copies: mutating the caller's tensors later must not move the
    # engine's environment
    return tuple(
        t.detach().to(device=device, dtype=torch.float32,
                      copy=True).contiguous() for t in (env_A, env_B))


# -- observation normaliser -------------------------------------------------
def normaliser(obs_sum, obs_sumsq, obs_count):
    """(obs_mu, obs_nu) from the running sums; row-wise on stacked state
    (obs_count ``[P][1]`` broadcasts over the 4 dims)."""
    count = obs_count.clamp_min(1.0)
    obs_mu = (obs_sum / count).contiguous()
    var = obs_sumsq / count - obs_mu ** 2
    return obs_mu, var.clamp_min(1e-2).contiguous()


class ObsNormaliser:
    """The running obs normalisation of an engine with ``cfg`` and
    ``device``: the sums a rollout reports are merged after each step and
    ``obs_mu`` / ``obs_nu`` applied from the next one on."""

    def _init_normaliser(self, *lead):
        """Allocate the state; ``lead`` stacks it, ``[P][4]`` / ``[P][1]``."""
        n, device = self.cfg.obs_dim, self.device
        self.obs_sum = torch.zeros(*lead, n, device=device)
        self.obs_sumsq = torch.zeros(*lead, n, device=device)
        self.obs_count = torch.zeros(*lead, 1, device=device)
        self.obs_mu = torch.zeros(*lead, n, device=device)
        self.obs_nu = torch.ones(*lead, n, device=device)

    def _refresh_normaliser(self):
        self.obs_mu, self.obs_nu = normaliser(self.obs_sum, self.obs_sumsq,
                                              self.obs_count)

    def _merge_obs_stat(self, obs_stat):
        """``obs_stat[..., 9]``: sum[4], sum of squares[4], count."""
        n = self.cfg.obs_dim
        self.obs_sum += obs_stat[..., :n]
        self.obs_sumsq += obs_stat[..., n:2 * n]
        self.obs_count += obs_stat[..., 2 * n:]
        self._refresh_normaliser()

    def _obs_state(self):
        return {
            "obs_sum": self.obs_sum.cpu(),
            "obs_sumsq": self.obs_sumsq.cpu(),
            "obs_count": self.obs_count.cpu(),
        }

    def _load_obs_state(self, state):
        self.obs_sum.copy_(state["obs_sum"].to(self.device))
        self.obs_sumsq.copy_(state["obs_sumsq"].to(self.device))
        self.obs_count.copy_(state["obs_count"].to(self.device))
        self._refresh_normaliser()


# -- update -----------------------------------------------------------------
def adam_ascent(theta, adam_m, adam_v, grad, t_step, cfg):
    """One Adam step up ``grad`` (fitness is maximised), in place on
    ``theta`` and the moments; ``t_step`` counts this step.  Elementwise, so
    row views and stacked ``[P][N]`` state take it as they are."""
    b1, b2 = cfg.adam_beta1, cfg.adam_beta2
    adam_m.mul_(b1).add_(grad, alpha=1 - b1)
    adam_v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
    mhat = adam_m / (1 - b1 ** t_step)
    vhat = adam_v / (1 - b2 ** t_step)
    theta.add_(cfg.lr * mhat / (vhat.sqrt() + cfg.adam_eps))


# -- act() ------------------------------------------------------------------
def act_input(engine, obs, obs_mask=None):
    """Raw observations ``obs[n][4]`` as the rollout kernels present them to
    the policy: ``(obs - mu) * rsqrt(nu + 1e-4)`` clamped to +-5 in fp32,
    the dims whose bit of ``obs_mask`` is 0 set to 0."""
    obs_dim = engine.cfg.obs_dim
    if not torch.is_tensor(obs):
        raise TypeError("obs must be a tensor, got %s" % type(obs).__name__)
    if obs.dim() != 2 or obs.shape[1] != obs_dim:
        raise ValueError("obs must be [n, %d], got %s"
                         % (obs_dim, tuple(obs.shape)))
    if obs.dtype != torch.float32:
        raise TypeError("obs must be torch.float32, got %s" % obs.dtype)
    if obs.device != engine.theta.device:
        raise TypeError("obs is on %s, the engine on %s"
                        % (obs.device, engine.theta.device))
    rstd = torch.rsqrt(engine.obs_nu + 1e-4)
    x = ((obs - engine.obs_mu) * rstd).clamp_(-5.0, 5.0)
    if obs_mask is not None:
        visible = torch.tensor(
            [(obs_mask >> d) & 1 for d in range(obs_dim)],
            dtype=torch.float32, device=obs.device)
        x = x * visible
    return x.contiguous()


# -- checkpoint files ---------------------------------------------------------
# (assigned as methods by the engines that have them)
def save(engine, path):
    torch.save(engine.state_dict(), path)


def load(engine, path):
    engine.load_state_dict(torch.load(path, weights_only=False))


# -- ESEngine's iteration on one GPU, the rollout swapped ---------------------
class RolloutESEngine(ObsNormaliser):
    nparams = None   # length of theta, for es_grad's noise
    _range = None    # tracing range of the rollout launch

    def __init__(self, config, device, env_params):
        self.cfg = config
        if device is None:
            device = torch.device("cuda", 0)
        self.device = device
        if config.pop_per_gpu % 2:
            raise ValueError("pop_per_gpu must be even (antithetic pairs)")
        self.pop_total = config.pop_per_gpu

        self.theta = self._init_theta()
        self.adam_m = torch.zeros_like(self.theta)
        self.adam_v = torch.zeros_like(self.theta)
        self.t_step = 0

        self._resolve_env(env_params)
        self._init_normaliser()

    def _resolve_env(self, env_params):
        """Keep the environment ``_rollout`` runs on; the synthetic linear
        one unless the engine has another."""
        self.env_A, self.env_B = resolve_env(self.cfg, self.device,
                                             env_params)

    def _init_theta(self):
        """The initial flat theta ``[nparams]`` on ``self.device``."""
        raise NotImplementedError

    def _rollout(self, sigma, iteration, horizon, pop):
        """``(fitness[pop], obs_stat[9])`` of members 0 .. pop - 1."""
        raise NotImplementedError

    def step(self, iteration=None):
        cfg = self.cfg
        if iteration is None:
            iteration = self.t_step
        pop = cfg.pop_per_gpu
        with tracing.range(self._range):
            fitness, obs_stat = self._rollout(cfg.sigma, iteration,
                                              cfg.horizon, pop)
        ranks = ops.centered_rank(fitness)
        wpair = (ranks[0::2] - ranks[1::2]).contiguous()
        with tracing.range("es.grad"):
            grad = ops.es_grad(wpair, 0, pop // 2, cfg.seed, iteration,
                               self.device, nparams=self.nparams)
        grad /= float(pop) * cfg.sigma

        self.t_step += 1
        adam_ascent(self.theta, self.adam_m, self.adam_v, grad, self.t_step,
                    cfg)
        self._merge_obs_stat(obs_stat)
        return {
            "fitness_mean": float(fitness.mean()),
            "fitness_max": float(fitness.max()),
            "grad_norm": float(grad.norm()),
            "rollouts": pop * cfg.envs_per_member,
            "env_steps": pop * cfg.envs_per_member * cfg.horizon,
        }

    def evaluate(self, horizon=None, iteration=None):
        """Mean return of the current, unperturbed theta over the 64
        episodes that ``step(iteration)`` starts from: the engine's rollout
        at ``sigma = 0`` with two members (one antithetic pair, both the
        plain theta).  Returns a 0-dim device tensor; changes nothing."""
        if horizon is None:
            horizon = self.cfg.horizon
        if iteration is None:
            iteration = self.t_step
        return self._rollout(0.0, iteration, horizon, 2)[0][0]

    def _state(self):
        """The state_dict() entries every engine of this kind has, in their
        checkpoint order; the engine appends its own and the config."""
        return {
            "theta": self.theta.cpu(),
            "adam_m": self.adam_m.cpu(),
            "adam_v": self.adam_v.cpu(),
            "t_step": self.t_step,
            **self._obs_state(),
        }

    def _load_state(self, state):
        self.theta.copy_(state["theta"].to(self.device))
        self.adam_m.copy_(state["adam_m"].to(self.device))
        self.adam_v.copy_(state["adam_v"].to(self.device))
        self.t_step = int(state["t_step"])
        self._load_obs_state(state)
