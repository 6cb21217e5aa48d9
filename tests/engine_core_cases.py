"""Shared by tests/test_engine_core.py and tests/gpu/test_engine_parity_gpu.py:
the host-side update sequences as every engine spelled them before
fiber_amd/es/_core.py, written out longhand, the shapes of the trajectory
tests and the checkpoint keys of every engine."""

from fiber_amd.es import ESConfig

# the smallest shapes with several antithetic pairs and a normaliser that
# step k hands to step k + 1
CFG = ESConfig(pop_per_gpu=8, horizon=4, seed=4321)
STEPS = 3
OBS_MASK = 0b0101
WIDE_HIDDEN = 128


# ---- the old sequences, longhand ------------------------------------------
def longhand_adam(theta, adam_m, adam_v, grad, t_step, cfg):
    b1, b2 = cfg.adam_beta1, cfg.adam_beta2
    adam_m.mul_(b1).add_(grad, alpha=1 - b1)
    adam_v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
    mhat = adam_m / (1 - b1 ** t_step)
    vhat = adam_v / (1 - b2 ** t_step)
    theta.add_(cfg.lr * mhat / (vhat.sqrt() + cfg.adam_eps))


def longhand_refresh(obs_sum, obs_sumsq, obs_count):
    count = obs_count.clamp_min(1.0)
    obs_mu = (obs_sum / count).contiguous()
    var = obs_sumsq / count - obs_mu ** 2
    return obs_mu, var.clamp_min(1e-2).contiguous()


def longhand_merge_1d(s, obs_stat, n=4):
    """ESEngine.step's lines on ``s.obs_*`` of shape [4] / [1]."""
    s.obs_sum += obs_stat[:n]
    s.obs_sumsq += obs_stat[n:2 * n]
    s.obs_count += obs_stat[2 * n]
    s.obs_mu, s.obs_nu = longhand_refresh(s.obs_sum, s.obs_sumsq,
                                          s.obs_count)


def longhand_merge_2d(s, obs_stat, n=4):
    """ESPopulation.step's lines on [P][4] / [P][1]."""
    s.obs_sum += obs_stat[:, :n]
    s.obs_sumsq += obs_stat[:, n:2 * n]
    s.obs_count += obs_stat[:, 2 * n:]
    s.obs_mu, s.obs_nu = longhand_refresh(s.obs_sum, s.obs_sumsq,
                                          s.obs_count)


# the state_dict keys of the commit before the shared core, in its order
_ES_KEYS = ("theta", "adam_m", "adam_v", "t_step", "obs_sum", "obs_sumsq",
            "obs_count")
CHECKPOINT_KEYS = {
    "ESEngine": _ES_KEYS + ("config",),
    "SNESEngine": _ES_KEYS + ("config", "sigma", "snes_config"),
    "RecurrentESEngine": _ES_KEYS + ("obs_mask", "config"),
    "LSTMESEngine": _ES_KEYS + ("obs_mask", "config"),
    "WideESEngine": _ES_KEYS + ("hidden", "config"),
    "NoveltyESEngine": (
        "thetas", "adam_m", "adam_v", "t_steps", "iteration", "obs_sum",
        "obs_sumsq", "obs_count", "archive", "archive_total", "agent_bc",
        "weight", "best_score", "stall", "generator", "config",
        "novelty_config"),
    "GAEngine": ("theta0", "lineage", "generation", "obs_sum", "obs_sumsq",
                 "obs_count", "config"),
    "SafeGAEngine": ("theta0", "lineage", "generation", "obs_sum",
                     "obs_sumsq", "obs_count", "config", "probe"),
    "MapElitesEngine": (
        "theta0", "me_lineage", "arch_fitness", "arch_bc", "arch_filled",
        "arch_born", "bc_lo", "bc_hi", "generation", "obs_sum", "obs_sumsq",
        "obs_count", "config"),
    "ESPopulation": ("theta", "adam_m", "adam_v", "obs_sum", "obs_sumsq",
                     "obs_count", "t_step", "seeds", "env_A", "env_B",
                     "config"),
}
