"""The engines built on fiber_amd/es/_core.py against a longhand loop of
the real ``ops`` calls and the update written out as every engine used to
spell it (tests/engine_core_cases.py), bit for bit, and the checkpoint keys
of the engines that only a GPU can construct."""

import dataclasses
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import engine_core_cases as C  # noqa: E402
from fiber_amd import ops  # noqa: E402
from fiber_amd.es import (ESEngine, ESPopulation, GAConfig, GAEngine,  # noqa: E402
                          LSTMESEngine, MapElitesConfig, MapElitesEngine,
                          NoveltyConfig, NoveltyESEngine, RecurrentESEngine,
                          SafeGAConfig, SafeGAEngine, SNESConfig, SNESEngine,
                          WideESEngine)
from fiber_amd.es.engine import init_theta, make_env_params  # noqa: E402
from fiber_amd.es.lstm import init_theta_lstm  # noqa: E402
from fiber_amd.es.recurrent import init_theta_gru  # noqa: E402
from fiber_amd.es.wide import init_theta_wide  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CFG, STEPS = C.CFG, C.STEPS
POP, SEED, H = CFG.pop_per_gpu, CFG.seed, CFG.horizon
SNES = SNESConfig().resolved(CFG)


def _rollouts(env_A, env_B, pop=POP):
    """kind -> rollout(theta, sigma, iteration, obs_mu, obs_nu): the call
    each engine makes, with the real kernels."""
    tail = (env_A, env_B)
    return {
        "es": lambda th, sg, it, mu, nu: ops.es_rollout_mlp(
            th, sg, SEED, it, H, 0, pop, mu, nu, *tail),
        "snes": lambda th, sg, it, mu, nu: ops.es_rollout_mlp_sigma(
            th, sg, SEED, it, H, 0, pop, mu, nu, *tail),
        "gru": lambda th, sg, it, mu, nu: ops.es_rollout_gru(
            th, sg, SEED, it, H, 0, pop, mu, nu, *tail, C.OBS_MASK),
        "lstm": lambda th, sg, it, mu, nu: ops.es_rollout_lstm(
            th, sg, SEED, it, H, 0, pop, mu, nu, *tail, C.OBS_MASK),
        "wide": lambda th, sg, it, mu, nu: ops.es_rollout_mlp_wide(
            th, C.WIDE_HIDDEN, sg, SEED, it, H, 0, pop, mu, nu, *tail),
    }


CASES = {
    "es": (lambda: ESEngine(CFG, ctx=None, device=DEV),
           lambda: init_theta(SEED, DEV), {}),
    "snes": (lambda: SNESEngine(CFG, device=DEV),
             lambda: init_theta(SEED, DEV),
             {"snes_config": dataclasses.asdict(SNES)}),
    "gru": (lambda: RecurrentESEngine(CFG, device=DEV, obs_mask=C.OBS_MASK),
            lambda: init_theta_gru(SEED, DEV), {"obs_mask": C.OBS_MASK}),
    "lstm": (lambda: LSTMESEngine(CFG, device=DEV, obs_mask=C.OBS_MASK),
             lambda: init_theta_lstm(SEED, DEV), {"obs_mask": C.OBS_MASK}),
    "wide": (lambda: WideESEngine(CFG, C.WIDE_HIDDEN, device=DEV),
             lambda: init_theta_wide(SEED, C.WIDE_HIDDEN, DEV),
             {"hidden": C.WIDE_HIDDEN}),
}


def longhand_run(kind):
    """STEPS iterations: the real rollout, rank and gradient launches and
    the written-out update.  Returns the state_dict fields (on the CPU) and
    the per-step (fitness_mean, fitness_max, grad_norm)."""
    cfg = CFG
    theta = CASES[kind][1]()
    adam_m, adam_v = torch.zeros_like(theta), torch.zeros_like(theta)
    t_step = 0
    s = types.SimpleNamespace(
        obs_sum=torch.zeros(4, device=DEV),
        obs_sumsq=torch.zeros(4, device=DEV),
        obs_count=torch.zeros(1, device=DEV),
        obs_mu=torch.zeros(4, device=DEV), obs_nu=torch.ones(4, device=DEV))
    rollout = _rollouts(*make_env_params(SEED, DEV))[kind]
    sigma = cfg.sigma
    if kind == "snes":
        sigma = torch.full((ops.NPARAMS,), float(cfg.sigma),
                           dtype=torch.float32, device=DEV)
    stats = []
    for _ in range(STEPS):
        iteration = t_step
        fitness, obs_stat = rollout(theta, sigma, iteration, s.obs_mu,
                                    s.obs_nu)
        ranks = ops.centered_rank(fitness)
        wpair = (ranks[0::2] - ranks[1::2]).contiguous()
        if kind == "snes":
            wsum = (ranks[0::2] + ranks[1::2]).contiguous()
            grad, g_sig = ops.es_grad_sigma(wpair, wsum, 0, POP // 2, SEED,
                                            iteration, DEV)
        elif kind == "es":
            grad = ops.es_grad(wpair, 0, POP // 2, SEED, iteration, DEV)
        else:
            grad = ops.es_grad(wpair, 0, POP // 2, SEED, iteration, DEV,
                               nparams=theta.numel())
        grad /= float(POP) * cfg.sigma
        t_step += 1
        C.longhand_adam(theta, adam_m, adam_v, grad, t_step, cfg)
        if kind == "snes":
            sigma.mul_(torch.exp(g_sig * (0.5 * SNES.lr_sigma / POP))
                       ).clamp_(SNES.sigma_min, SNES.sigma_max)
        C.longhand_merge_1d(s, obs_stat)
        stats.append((float(fitness.mean()), float(fitness.max()),
                      float(grad.norm())))
    state = {"theta": theta.cpu(), "adam_m": adam_m.cpu(),
             "adam_v": adam_v.cpu(), "t_step": t_step,
             "obs_sum": s.obs_sum.cpu(), "obs_sumsq": s.obs_sumsq.cpu(),
             "obs_count": s.obs_count.cpu(),
             "config": dataclasses.asdict(cfg)}
    if kind == "snes":
        state["sigma"] = sigma.cpu()
    state["obs_mu"], state["obs_nu"] = s.obs_mu.cpu(), s.obs_nu.cpu()
    return state, stats


def _assert_same(got, want, what):
    assert set(got) == set(want), what
    for key, value in want.items():
        if torch.is_tensor(value):
            assert torch.equal(got[key], value), (what, key)
        else:
            assert got[key] == value, (what, key)


@pytest.mark.parametrize("kind", list(CASES))
def test_engine_equals_longhand(kind):
    want, want_stats = longhand_run(kind)
    again, again_stats = longhand_run(kind)
    # the kernels reduce in a fixed order: the reference repeats itself
    _assert_same(again, want, "longhand run twice")
    assert again_stats == want_stats
    assert want["t_step"] == STEPS
    assert float(want["obs_count"]) == STEPS * POP * 64 * H
    assert float(want["adam_v"].max()) > 0.0

    eng = CASES[kind][0]()
    stats = [eng.step() for _ in range(STEPS)]
    got = eng.state_dict()
    assert tuple(got) == C.CHECKPOINT_KEYS[type(eng).__name__]
    got["obs_mu"], got["obs_nu"] = eng.obs_mu.cpu(), eng.obs_nu.cpu()
    want.update(CASES[kind][2])
    _assert_same(got, want, kind)
    for st, (fmean, fmax, gnorm) in zip(stats, want_stats):
        assert (st["fitness_mean"], st["fitness_max"],
                st["grad_norm"]) == (fmean, fmax, gnorm)
        assert st["rollouts"] == POP * 64
        assert st["env_steps"] == POP * 64 * H
    if kind not in ("es", "snes"):
        # evaluate(): the engine's rollout at sigma = 0 with two members
        mu, nu = eng.obs_mu, eng.obs_nu
        ref = _rollouts(eng.env_A, eng.env_B, 2)[kind](
            eng.theta, 0.0, eng.t_step, mu, nu)[0]
        val = eng.evaluate()
        assert val.dim() == 0 and torch.equal(val, ref[0])
        assert torch.equal(eng.state_dict()["theta"], want["theta"])


# ---- checkpoint keys of the engines that need the device to exist ----------
def _others():
    envs = [make_env_params(100 + p, "cpu") for p in range(2)]
    return {
        "NoveltyESEngine": lambda: NoveltyESEngine(
            CFG, NoveltyConfig(k=2, meta_size=2, archive_capacity=8),
            device=DEV),
        "GAEngine": lambda: GAEngine(
            GAConfig(pop=8, truncation=2, horizon=H, seed=SEED), device=DEV),
        "SafeGAEngine": lambda: SafeGAEngine(
            SafeGAConfig(pop=8, truncation=2, horizon=H, seed=SEED),
            device=DEV),
        "MapElitesEngine": lambda: MapElitesEngine(
            MapElitesConfig(pop=8, bins=(2, 2, 1, 1), horizon=H, seed=SEED),
            device=DEV),
        "ESPopulation": lambda: ESPopulation(CFG, [11, 12], envs, device=DEV),
    }


@pytest.mark.parametrize("name", list(_others()))
def test_checkpoint_keys_and_normaliser_restore(name):
    make = _others()[name]
    eng = make()
    assert type(eng).__name__ == name
    for _ in range(2):
        eng.step()
    state = eng.state_dict()
    assert tuple(state) == C.CHECKPOINT_KEYS[name]
    mu, nu = C.longhand_refresh(eng.obs_sum, eng.obs_sumsq, eng.obs_count)
    assert torch.equal(eng.obs_mu, mu) and torch.equal(eng.obs_nu, nu)
    assert float(eng.obs_count.reshape(-1)[0]) == 2 * 8 * 64 * H
    other = make()
    other.load_state_dict(state)
    for f in ("obs_sum", "obs_sumsq", "obs_count", "obs_mu", "obs_nu"):
        assert torch.equal(getattr(other, f), getattr(eng, f)), f
    again = other.state_dict()
    assert tuple(again) == C.CHECKPOINT_KEYS[name]
    for key in ("obs_sum", "obs_sumsq", "obs_count"):
        assert torch.equal(again[key], state[key]), key
