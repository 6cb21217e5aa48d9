"""The wide MLP policy kernels (hidden 128 / 256) against
fiber_amd.es.wide_oracle (fp64), and the engine against a hand composition
of the ops.  Every test prints its worst error / tolerance ratio
(profiles/wide_mlp.md records them)."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import wide_cases as C  # noqa: E402
from fiber_amd import ops  # noqa: E402
from fiber_amd.es import ESConfig, WideESEngine, init_theta_wide  # noqa: E402
from fiber_amd.es import wide_oracle as W  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
hidden_cases = pytest.mark.parametrize("hidden", C.HIDDEN)


def _ratio(got, want, tol):
    return float((np.abs(got.astype(np.float64) - want) / tol).max())


def _launch(world, hidden, sigma, horizon, offset, pop, final=True):
    theta, mu, nu, env_A, env_B = world
    out = ops.es_rollout_mlp_wide(theta, hidden, sigma, C.SEED, C.ITER,
                                  horizon, offset, pop, mu, nu, env_A, env_B,
                                  return_final=final)
    return [t.cpu().numpy() for t in out]


# ---- 1. one rollout step, restarted from the kernel's own state ------------

@hidden_cases
@pytest.mark.parametrize("h", C.HORIZONS)
@pytest.mark.parametrize("sigma", C.SIGMAS)
def test_rollout_step_matches_oracle(hidden, h, sigma):
    world = C.world(hidden, DEV)
    theta, mu, nu, env_A, env_B = [t.cpu().numpy() for t in world]
    pop = C.POP
    f0, st0, s0 = _launch(world, hidden, sigma, h, C.OFFSET, pop)
    f1, st1, s1 = _launch(world, hidden, sigma, h + 1, C.OFFSET, pop)
    if h == 0:
        init = C.init_state()
        assert (np.abs(s0 - init) <= (W.Z_REL + W.U) * np.abs(init)).all()
        assert not f0.any() and not st0.any()
    worst, n_close = {}, 0
    for m in C.MEMBERS:
        pol = C.member_policy(theta, hidden, sigma, m)
        x, x_slack = W.observe(s0[m], mu, nu)
        logits, tol_l = W.forward(pol, x, x_slack)
        act = logits[:, 1] > logits[:, 0]
        close = np.abs(logits[:, 1] - logits[:, 0]) <= tol_l.sum(-1)
        n_close += int(close.sum())
        sa, tol_s = W.env_step(s0[m], act, env_A, env_B)
        sb, _ = W.env_step(s0[m], ~act, env_A, env_B)
        ra = (np.abs(s1[m] - sa) / tol_s).max(-1)
        rb = (np.abs(s1[m] - sb) / tol_s).max(-1)
        worst["s"] = max(worst.get("s", 0),
                         float(np.where(close, np.minimum(ra, rb), ra).max()))
        # fitness increment, from the kernel's own states
        s64 = s1[m].astype(np.float64)
        rew = 64.0 - W.C01 * (s64 * s64).sum()
        # per step: 3 roundings of 0.1*s*s and the subtract, then h+1 adds
        # per thread, 3 + 6 adds across dims and envs, on sums <= mag
        mag = 64.0 * (h + 1) + W.C01 * (s64 * s64).sum() * (h + 1)
        worst["f"] = max(worst.get("f", 0), abs(
            64.0 * (float(f1[m]) - float(f0[m])) - rew)
            / ((h + 14) * W.U * mag))
    assert n_close <= C.CLOSE_CAP * 64 * len(C.MEMBERS)
    # obs_stat[h+1] - obs_stat[h] = the states at step h, over all members.
    # Each launch rounds on its own.  A term passes h + 1 adds in its
    # thread, 6 in the shuffle tree over the envs and 1 + 8 in
    # obs_stat_reduce (pop <= 256), and a square is rounded once before it
    # enters: h + 17 roundings, each within U of a partial sum that never
    # exceeds sum|terms|.  For the squares that is the slot itself; for the
    # n = 64 pop (h + 1) plain terms it is at most sqrt(n * sumsq).  The
    # shorter launch's bound is no larger, hence the 2.
    s64 = s0.astype(np.float64)
    want = np.concatenate([s64.sum((0, 1)), (s64 * s64).sum((0, 1))])
    sumsq = st1[4:8].astype(np.float64)
    big = np.concatenate([np.sqrt(64.0 * pop * (h + 1) * sumsq), sumsq])
    worst["stat"] = float((np.abs(
        st1[:8].astype(np.float64) - st0[:8] - want)
        / (2.0 * (h + 17) * W.U * big)).max())
    assert st0[8] == 64 * pop * h and st1[8] == 64 * pop * (h + 1)
    print("rollout_step H=%d h=%d sigma=%g: %s close %d"
          % (hidden, h, sigma, worst, n_close))
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- 2. mlp_policy_forward_wide against forward ----------------------------

@hidden_cases
@pytest.mark.parametrize("batch", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("scale", [1.0, 8.0])
def test_forward_matches_oracle(hidden, batch, scale):
    theta = init_theta_wide(11, hidden, "cpu") * scale
    gen = torch.Generator().manual_seed(batch)
    x = torch.randn(batch, 4, generator=gen).bfloat16().float()
    logits = ops.mlp_policy_forward_wide(theta.to(DEV), hidden, x.to(DEV))
    want, tol = W.forward(W.make_policy(theta.numpy(), hidden), x.numpy())
    r = _ratio(logits.cpu().numpy(), want, tol)
    print("forward H=%d b=%d x%g: %.3f" % (hidden, batch, scale, r))
    assert r <= 1.0


# ---- 3. bits ---------------------------------------------------------------

@hidden_cases
def test_outputs_offset_and_repeats_do_not_change_bits(hidden):
    world = C.world(hidden, DEV)
    f, st, s = _launch(world, hidden, 0.05, 9, 0, 8)
    f_plain, st_plain = _launch(world, hidden, 0.05, 9, 0, 8, final=False)
    assert f.tobytes() == f_plain.tobytes()
    assert st.tobytes() == st_plain.tobytes()
    f_off, _st, s_off = _launch(world, hidden, 0.05, 9, 2, 6)
    assert f_off.tobytes() == f[2:].tobytes()
    assert s_off.tobytes() == s[2:].tobytes()
    again = _launch(world, hidden, 0.05, 9, 0, 8)
    assert [a.tobytes() for a in again] == [f.tobytes(), st.tobytes(),
                                            s.tobytes()]
    assert len(set(f.tolist())) > 1        # the members do differ
    f_zero = _launch(world, hidden, 0.0, 9, 0, 8)[0]
    assert (f_zero[0::2].view(np.uint32) == f_zero[1::2].view(np.uint32)).all()


# ---- 4. engine glue --------------------------------------------------------

def _engine_bits(e):
    return [t.cpu().numpy().tobytes() for t in (
        e.theta, e.adam_m, e.adam_v, e.obs_sum, e.obs_sumsq, e.obs_count,
        e.obs_mu, e.obs_nu)]


@hidden_cases
def test_engine_step_is_the_hand_composition(hidden, tmp_path):
    cfg = ESConfig(pop_per_gpu=32, horizon=6, seed=99)
    eng = WideESEngine(cfg, hidden, device=DEV)
    theta = eng.theta.clone()
    fit, stat = ops.es_rollout_mlp_wide(
        theta, hidden, cfg.sigma, cfg.seed, 0, cfg.horizon, 0, 32,
        eng.obs_mu, eng.obs_nu, eng.env_A, eng.env_B)
    ranks = ops.centered_rank(fit)
    grad = ops.es_grad((ranks[0::2] - ranks[1::2]).contiguous(), 0, 16,
                       cfg.seed, 0, DEV, nparams=ops.wide_nparams(hidden))
    grad /= 32.0 * cfg.sigma
    assert float(grad.norm()) > 0.0
    m = torch.zeros_like(theta).add_(grad, alpha=1 - cfg.adam_beta1)
    v = torch.zeros_like(theta).addcmul_(grad, grad,
                                         value=1 - cfg.adam_beta2)
    theta += cfg.lr * (m / (1 - cfg.adam_beta1)) / (
        (v / (1 - cfg.adam_beta2)).sqrt() + cfg.adam_eps)
    eng.step()
    assert torch.equal(eng.theta, theta)
    assert torch.equal(eng.adam_m, m) and torch.equal(eng.adam_v, v)
    assert torch.equal(eng.obs_sum, stat[:4])
    assert torch.equal(eng.obs_sumsq, stat[4:8])
    assert torch.equal(eng.obs_count, stat[8:])

    # a reloaded engine takes the same next step
    path = str(tmp_path / "wide.pt")
    eng.save(path)
    twin = WideESEngine(cfg, hidden, device=DEV)
    twin.load(path)
    assert twin.state_dict()["hidden"] == hidden
    eng.step()
    twin.step()
    assert _engine_bits(twin) == _engine_bits(eng)
    assert torch.isfinite(eng.evaluate())
    other = WideESEngine(cfg, 384 - hidden, device=DEV)
    with pytest.raises(ValueError):
        other.load_state_dict(eng.state_dict())

    # act() is normalise + mlp_policy_forward_wide
    obs = torch.randn(70, 4, device=DEV)
    actions, logits = eng.act(obs, return_logits=True)
    x = ((obs - eng.obs_mu) * torch.rsqrt(eng.obs_nu + 1e-4)).clamp(-5, 5)
    want = ops.mlp_policy_forward_wide(eng.theta, hidden, x.contiguous())
    assert torch.equal(logits, want)
    assert torch.equal(actions, (want[:, 1] > want[:, 0]).long())


def test_ring_and_hidden_64_are_refused():
    cfg = ESConfig(pop_per_gpu=8)
    with pytest.raises(NotImplementedError):
        WideESEngine(cfg, 128, ctx=object(), device=DEV)
    with pytest.raises(ValueError, match="es_rollout_mlp"):
        WideESEngine(cfg, 64, device=DEV)
    world = C.world(128, DEV)
    with pytest.raises(ValueError, match="es_rollout_mlp"):
        ops.es_rollout_mlp_wide(world[0], 64, 0.05, 1, 0, 4, 0, 2, *world[1:])
    with pytest.raises(ValueError):       # a 128-wide theta is not 256-wide
        ops.es_rollout_mlp_wide(world[0], 256, 0.05, 1, 0, 4, 0, 2,
                                *world[1:])
